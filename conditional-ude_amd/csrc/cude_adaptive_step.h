// Pieces of the adaptive Tsit5 step that the kernels with unrolled stages state once: cude_adaptive_unrolled.hip (c-peptide,
// one wave per 64 subjects), cude_adaptive_team.hip (c-peptide, a team of waves per 64 subjects) and
// cude_adaptive_unrolled_supp.hip (suppression model; it takes the error estimate only).  Functions of the kernels' own
// rows and locals; nothing here asks which kernel is calling.  The team kernel's waves reach the same accept / reject
// decisions because they judge a trial step by THIS estimate on the same values (tests/test_gpu_round5.py holds it to
// the one-wave kernel bit for bit).
// Only what compiles to the same registers and the same arithmetic in its callers is here.  The six stages, the `saveat`
// interpolant and the bookkeeping around a trial step are still stated in each kernel: as shared functions they moved
// the c-peptide kernels' register allocation and spills (profiles/adaptive_step_shared.txt).
#pragma once
#include "cude_adaptive.h"

namespace cude {

// stage adjoints of the step being reversed (c-peptide kernels): registers, or LDS rows for the networks whose gradient
// accumulators fill the register file.  One threshold for the one-wave kernel and the team's scribe: a
// -DCUDE_ADAPT_BLDS_NACC=... build moves both, and with them the LDS size of either launch
#ifndef CUDE_ADAPT_BLDS_NACC
#define CUDE_ADAPT_BLDS_NACC 40
#endif
template <class M, bool GRAD>
constexpr bool adjoints_in_lds() { return GRAD && M::NetT::NACC > CUDE_ADAPT_BLDS_NACC; }

// scaled error estimate of the trial step: rms of dt sum_j bt_j K_j / (abstol + reltol max(|y|, |ynew|))
template <int NS>
__device__ __forceinline__ double tsit5_error_estimate(const double (&K)[7][NS], const double (&y)[NS], const double (&ynew)[NS],
                                                       double dt, double abstol, double reltol) {
    double ev[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) {
        double e = 0.0;
#pragma unroll
        for (int j = 0; j < 7; j++) e = fma(TS_BT[j], K[j][s], e);
        ev[s] = dt * e / fma(reltol, fmax(fabs(y[s]), fabs(ynew[s])), abstol);
    }
    return rms(ev, NS);
}

// most accepted steps of any lane of the wave: the trip count of the reverse sweep
__device__ __forceinline__ int adaptive_wave_max(int n) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) n = max(n, __shfl_xor(n, off, 64));
    return n;
}

// tape entry a lane reads in iteration n of the reverse sweep: a lane with fewer accepted steps idles on its last entry
// with zero adjoints until its own steps come up; a lane with none (parked from the start) reads entry 0, which the
// kernels fill with finite numbers before the first step
__device__ __forceinline__ int tape_entry(int n, int n_acc) { return n < n_acc ? n : (n_acc > 0 ? n_acc - 1 : 0); }

}  // namespace cude
