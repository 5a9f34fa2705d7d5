// Adaptive Tsit5 ensemble kernels for gfx950 -- what the reference actually runs.
//
// Replaces (reference repo paths; the solver itself is OrdinaryDiffEq, third-party, restated here from its documented
// defaults; the reference's stored objectives pin this restatement, tests/test_gpu_known_answers.py):
//   solve(model.problem, p = theta, saveat = timepoints, save_idxs = 1)          src/parameter-estimation.jl:59
//   solve(prob, saveat = timepoints, save_idxs = 1)                              src/saem.jl:52
//   solve(ensemble, Tsit5(), EnsembleThreads(); saveat, trajectories = N)        suppression/src/suppression_model.jl:113,123
// i.e. Tsit5 with abstol 1e-6 / reltol 1e-3, the PI step controller (beta1 = 7/50, beta2 = 2/25, gamma = 0.9,
// qmin = 0.2, qmax = 10), Hairer's initial-step heuristic, `saveat` through the free 4th-order interpolant, failure
// (non-finite error estimate, more than 1e5 steps) => +Inf loss.  Selected by cude_config.n_steps = 0: loss,
// per-subject SSE, trajectories, dense output, profiles, screening, Metropolis E-step, and -- GRAD -- the gradient.
//
// Gradient of the adaptive solve = what the reference's AutoForwardDiff computes (src/parameter-estimation.jl:165,
// suppression_model.jl:155): under ForwardDiff only p = theta carries partials, tspan and dt stay Float64, so the
// derivative is that of the accepted step sequence as fixed arithmetic (controller and initial-step heuristic are not
// differentiated).  Here: the forward sweep writes every accepted step to a per-subject tape in HBM ([step][rows]
// [subject], coalesced) -- (t_n, dt_n, y_n) for the suppression model, whose reverse sweep re-runs the stage evaluations
// from y_n; dt_n ALONE (8 B per step) for the c-peptide models, whose Jacobian is constant: their reverse sweep needs
// the stage TIMES only and steps back from the final time, t_n = t_{n+1} - dt_n (within an ulp of the forward sweep's
// t_n: the forward sum is not exactly invertible; 1e-16 relative in a network input) -- and the reverse sweep walks the
// tape backwards and applies the stage VJPs in reverse order, including the `saveat` interpolation weights of the
// observations that fell into the step.  (OrdinaryDiffEq's error norm under duals also weighs the partials -- its
// documented behaviour -- so the reference's accepted steps during a gradient call can differ from those of a plain
// solve; the sequence here is the plain solve's.)  Lanes with more accepted steps than the tape holds fail (+Inf).
//
// One lane = one subject, each with its own (t, dt, controller state): the lanes of a wave walk the same sequence of
// phases (k1, the f1 probe of the initial step, then stages 2..7 of step after step) with ONE inlined network body;
// a lane that has reached t_end stops committing and the wave leaves when all of its lanes are done (or after the
// solver's own step limit, so every wave terminates).
#include "cude_adaptive_body.h"

namespace cude {


// ---------------------------------------------------------------------------------- dispatch
template <class M, bool IS_CPEP>
static hipError_t launch_adaptive(const typename M::Args& a, int extra_rows, bool grad, hipStream_t s) {
    const int64_t nblocks = grad ? (a.N + kBlock - 1) / kBlock : launch_blocks(a);
    const size_t lds = sizeof(double) * (size_t)(adaptive_rows<M>(grad) + extra_rows) * kBlock;
    const unsigned n_sets = a.n_sets > 0 ? (unsigned)a.n_sets : 1u;
    if (grad && (a.tape == nullptr || a.tape_cap < 1 || a.g_cond == nullptr)) return hipErrorInvalidValue;
    if (grad && a.lane_rows != nullptr) {
        hipLaunchKernelGGL((adaptive_kernel<M, IS_CPEP, true, true>), dim3((unsigned)nblocks, n_sets), dim3(kBlock), lds, s, a);
    } else if (grad) {
        hipLaunchKernelGGL((adaptive_kernel<M, IS_CPEP, true>), dim3((unsigned)nblocks, n_sets), dim3(kBlock), lds, s, a);
    } else {
        hipLaunchKernelGGL((adaptive_kernel<M, IS_CPEP, false>), dim3((unsigned)nblocks, n_sets), dim3(kBlock), lds, s, a);
    }
    return hipGetLastError();
}

// outputs-only launch of the suppression model (dense output, SuppArgs::T_data > 0; M = SuppAdOut): forward only
template <class M>
static hipError_t launch_adaptive_out(const SuppArgs& a, hipStream_t s) {
    const int64_t nblocks = launch_blocks(a);
    const size_t lds = sizeof(double) * (size_t)adaptive_rows<M>(false) * kBlock;
    const unsigned n_sets = a.n_sets > 0 ? (unsigned)a.n_sets : 1u;
    if (a.traj == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL((adaptive_kernel<M, false, false>), dim3((unsigned)nblocks, n_sets), dim3(kBlock), lds, s, a);
    return hipGetLastError();
}

#ifndef CUDE_AD_PART
#define CUDE_AD_PART 0
#endif
#if CUDE_AD_PART == 0
hipError_t launch_cpep_adaptive(const NetShape& net, bool grad, const CpepArgs& a, hipStream_t s) {
    if (a.TG < 2 || a.TG > kMaxObs || a.T < 1) return hipErrorInvalidValue;
    if (grad && a.obs == nullptr) return hipErrorInvalidValue;
#ifndef CUDE_ADAPT_ONE_BODY                        /* (A/B builds: tools/abl_adaptive_bits.py) */
    if (!net.general() && a.TG <= kUnrolledKnots) {
        hipError_t e = launch_cpep_adaptive_team(net, grad, a, s);      // small launches: five waves per 64 subjects
        if (e != hipErrorNotSupported) return e;
        e = launch_cpep_adaptive_unrolled(net, grad, a, s);
        if (e != hipErrorNotSupported) return e;
    }
#endif
    if (net.symbolic())
        return a.cond_raw ? launch_adaptive<CpepAd<MmProd<true>>, true>(a, a.TG, grad, s)
                          : launch_adaptive<CpepAd<MmProd<false>>, true>(a, a.TG, grad, s);
    if (net.general())
        return visit_cpep_general(net, hipErrorInvalidValue, [&](auto sh, auto act) {
            return launch_adaptive<CpepAd<CpepNetG<sh.nin, sh.width, sh.depth, act.hact, act.oact>>, true>(a, a.TG, grad, s);
        });
    hipError_t e = visit_cpep_shapes_0(net, hipErrorNotSupported, [&](auto sh) {
        return launch_adaptive<CpepAd<Mlp<sh.nin, sh.width, sh.depth, 1>>, true>(a, a.TG, grad, s);
    });
    if (e == hipErrorNotSupported) e = launch_cpep_adaptive_part1(net, grad, a, s);
    if (e == hipErrorNotSupported) e = launch_cpep_adaptive_part2(net, grad, a, s);
    return e == hipErrorNotSupported ? hipErrorInvalidValue : e;
}

hipError_t launch_supp_adaptive(const NetShape& net, bool grad, const SuppArgs& a, hipStream_t s) {
    if (net.nin != 4 || a.T < 1 || (a.T_data > 0 && grad)) return hipErrorInvalidValue;
#ifndef CUDE_ADAPT_ONE_BODY
    if (!net.general()) {
        const hipError_t e = launch_supp_adaptive_unrolled(net, grad, a, s);
        if (e != hipErrorNotSupported) return e;
    }
#endif
    if (net.general())
        return visit_supp_general(net, hipErrorInvalidValue, [&](auto sh, auto act) {
            constexpr int W = sh.width, D = sh.depth, HA = act.hact, OA = act.oact;
            return a.T_data > 0 ? launch_adaptive_out<SuppAdOut<W, D, HA, OA>>(a, s) : launch_adaptive<SuppAd<W, D, HA, OA>, false>(a, 0, grad, s);
        });
    // (the one-body kernel of the shapes the unrolled kernel does not cover: cude_shapes.h CUDE_SUPP_AD_SHAPES)
    return visit_supp_ad_shapes(net, hipErrorInvalidValue, [&](auto sh) {
        return a.T_data > 0 ? launch_adaptive_out<SuppAdOut<sh.width, sh.depth>>(a, s)
                            : launch_adaptive<SuppAd<sh.width, sh.depth>, false>(a, 0, grad, s);
    });
}
#elif CUDE_AD_PART == 1
hipError_t launch_cpep_adaptive_part1(const NetShape& net, bool grad, const CpepArgs& a, hipStream_t s) {
    return visit_cpep_shapes_1(net, hipErrorNotSupported, [&](auto sh) {
        return launch_adaptive<CpepAd<Mlp<sh.nin, sh.width, sh.depth, 1>>, true>(a, a.TG, grad, s);
    });
}
#else
hipError_t launch_cpep_adaptive_part2(const NetShape& net, bool grad, const CpepArgs& a, hipStream_t s) {
    return visit_cpep_shapes_2(net, hipErrorNotSupported, [&](auto sh) {
        return launch_adaptive<CpepAd<Mlp<sh.nin, sh.width, sh.depth, 1>>, true>(a, a.TG, grad, s);
    });
}
#endif

}  // namespace cude
