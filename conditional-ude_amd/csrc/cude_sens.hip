// Forward-mode (tangent-linear) ensemble solves for gfx950: every subject's trajectory together with its derivative with
// respect to the subject's own conditional parameter (cude_sensitivity).
//
// Replaces (reference repo paths): the partials every solve of the reference carries under ForwardDiff --
//   sensealg = ForwardDiffSensitivity()                                  src/parameter-estimation.jl:59
//   AutoForwardDiff() through `solve`                                    src/parameter-estimation.jl:165,370
//   the same through the suppression model's ensemble solve             suppression/src/suppression_model.jl:155
// restricted to the per-subject direction d/d(beta_i) resp. d/d(theta_i), which is what standard errors, Wald intervals
// and identifiability flags of a conditional parameter are built from.
//
// One lane = one subject, as cude_cpep.hip / cude_supp_dense.hip; no reduction over subjects except the (sum SSE, failures)
// pair.  The fixed-step sweeps themselves are in cude_tangent.h (cpep_tan_sweep / supp_tan_sweep), which the fused fits of
// cude_refine.hip call as well: the kernels here are prologue, one call with a functor that stores d u / d cond at the
// observation times, epilogue.  The network is evaluated in forward mode (Mlp::eval_jvp / MmProd::eval_jvp, cude_device.h):
// one sweep gives the value and the directional derivative, every weight column is read once for both.
//   * c-peptide models: the production does not depend on the state, so d prod / d beta is a FORCING of the linear tangent
//     system  s' = A s + [d q / d beta; 0]  -- the step's Runge-Kutta algebra simply runs a second time on (s, dq) with
//     f0 = 0.  Five evaluations per step, as the forward kernel.
//   * suppression model: the network reads the state, so the tangent needs the full JVP in x (the state's tangent) and in
//     the theta column (the first-layer offsets).  State 1 depends on no parameter: its tangent is exactly 0 and is not
//     carried; as in the forward kernels its value comes from the closed-form tables (SuppArgs::rho, obs_rho).
//   * adaptive mode: tangent policies (CpepAdTan / SuppAdTan, cude_adaptive.h) over the one-body kernel
//     (cude_adaptive_body.h), instantiated here.
// The networks are the exponential-form ones (no tanh table, no LDS biases): the types the adaptive kernels use.
//
// Failure convention (cude_simulate's): a subject with a non-finite input or a failed adaptive solve gets NaN in all its
// outputs and counts as failed; the other lanes' arithmetic does not depend on it.
//
// The file is compiled in parts (-DCUDE_SENS_PART=k, as cude_adaptive.hip): 0 = c-peptide fixed-step + the dispatchers,
// 1 = c-peptide adaptive, 2 = suppression fixed-step, 3 = suppression adaptive.
#include "cude_adaptive_body.h"
#include "cude_tangent.h"

namespace cude {

#ifndef CUDE_SENS_PART
#define CUDE_SENS_PART 0
#endif

hipError_t launch_cpep_sens_adaptive(const NetShape& net, const CpepSensArgs& a, hipStream_t s);
hipError_t launch_supp_sens_fixed(const NetShape& net, const SuppSensArgs& a, hipStream_t s);
hipError_t launch_supp_sens_adaptive(const NetShape& net, const SuppSensArgs& a, hipStream_t s);

// per-subject outputs behind a fixed-step solve (bad: NaN throughout)
template <int NS, class Args>
__device__ __forceinline__ void sens_finish(const Args& a, int64_t i, bool bad, double sse, double info, double score) {
    const double nan = __builtin_nan("");
    if (a.sse != nullptr) a.sse[i] = sse;
    if (a.out.info != nullptr) a.out.info[i] = bad ? nan : info;
    if (a.out.score != nullptr) a.out.score[i] = bad ? nan : score;
    if (bad && a.out.sens != nullptr)
        for (int q = 0; q < NS * a.T; q++) a.out.sens[(int64_t)NS * a.T * i + q] = nan;
}

#if CUDE_SENS_PART == 0
// ---------------------------------------------------------------------------------- c-peptide models, fixed step
// Net: Mlp<NIN, W, D, 1, false, false, HA, OA> or MmProd<RAW>.  NS = 3: + the cumulative-secretion quadrature state.
template <class Net, int NS>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2))) void cpep_sens_kernel(CpepSensArgs a) {
    constexpr int P = Net::P;
    extern __shared__ double smem[];
    double* s_q = smem;                         // [5][2][kBlock] stage forcings and their tangents
    double* s_red = smem + 10 * kBlock;         // [kRedRows][kBlock]
    const int lane = threadIdx.x;
    const int64_t gid = (int64_t)blockIdx.x * kBlock + lane;
    const bool active = gid < a.N;
    const int64_t i = active ? gid : a.N - 1;
    const int T = a.T;

    const CpepTanConst k = cpep_tan_load<Net>(a, i);
    const TanSums r = cpep_tan_sweep<Net, NS>(a, k, i, lane, a.cond[i], s_q, [&](int oi, double d1, double d2, double d3) {
        if (a.out.sens != nullptr && active) {
            double* tr = a.out.sens + (int64_t)NS * (oi + (int64_t)T * i);
            tr[0] = d1;
            tr[1] = d2;
            if (NS == 3) tr[2] = d3;
        }
    });
    const bool failed = !(fabs(r.sse) <= 1.79769313486231570815e308);   // NaN or Inf
    if (active) sens_finish<NS>(a, i, failed, r.sse, r.info, r.score);
    const double v2[2] = {active ? r.sse : 0.0, (active && failed) ? 1.0 : 0.0};
    block_reduce_store<2>(v2, s_red, a.partials + (int64_t)blockIdx.x * (P + 2) + P, lane);
}

template <class Net>
static hipError_t launch_cpep_fixed(int n_state, const CpepSensArgs& a, hipStream_t s) {
    const int64_t nblocks = (a.N + kBlock - 1) / kBlock;
    const size_t lds = sizeof(double) * (size_t)(10 + kRedRows) * kBlock;
    if (n_state == 2) hipLaunchKernelGGL((cpep_sens_kernel<Net, 2>), dim3((unsigned)nblocks), dim3(kBlock), lds, s, a);
    else hipLaunchKernelGGL((cpep_sens_kernel<Net, 3>), dim3((unsigned)nblocks), dim3(kBlock), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_cpep_sens(const NetShape& net, int n_state, const CpepSensArgs& a, hipStream_t s) {
    if (net.generic() || a.partials == nullptr || a.obs == nullptr || a.T < 1 || a.n_sets > 1) return hipErrorInvalidValue;
    if (a.S == 0) return n_state == 2 ? launch_cpep_sens_adaptive(net, a, s) : hipErrorInvalidValue;
    if (n_state != 2 && n_state != 3) return hipErrorInvalidValue;
    if (net.symbolic())
        return a.cond_raw ? launch_cpep_fixed<MmProd<true>>(n_state, a, s) : launch_cpep_fixed<MmProd<false>>(n_state, a, s);
    if (net.general())
        return visit_cpep_general(net, hipErrorInvalidValue, [&](auto sh, auto act) {
            return launch_cpep_fixed<CpepNetG<sh.nin, sh.width, sh.depth, act.hact, act.oact>>(n_state, a, s);
        });
    return visit_cpep_shapes(net, hipErrorInvalidValue, [&](auto sh) {
        return launch_cpep_fixed<Mlp<sh.nin, sh.width, sh.depth, 1>>(n_state, a, s);
    });
}

hipError_t launch_supp_sens(const NetShape& net, const SuppSensArgs& a, hipStream_t s) {
    if (net.nin != 4 || net.generic() || a.partials == nullptr || a.T < 1 || a.n_sets > 1 || a.T_data > 0) return hipErrorInvalidValue;
    return a.S == 0 ? launch_supp_sens_adaptive(net, a, s) : launch_supp_sens_fixed(net, a, s);
}

#elif CUDE_SENS_PART == 1
// ---------------------------------------------------------------------------------- c-peptide models, adaptive
template <class Net>
static hipError_t launch_cpep_tan(const CpepSensArgs& a, hipStream_t s) {
    using M = CpepAdTan<Net>;
    const int64_t nblocks = (a.N + kBlock - 1) / kBlock;
    const size_t lds = sizeof(double) * (size_t)(adaptive_rows<M>(false) + a.TG) * kBlock;
    hipLaunchKernelGGL((adaptive_kernel<M, true, false>), dim3((unsigned)nblocks), dim3(kBlock), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_cpep_sens_adaptive(const NetShape& net, const CpepSensArgs& a, hipStream_t s) {
    if (a.TG < 2 || a.TG > kMaxObs) return hipErrorInvalidValue;
    if (net.symbolic()) return a.cond_raw ? launch_cpep_tan<MmProd<true>>(a, s) : launch_cpep_tan<MmProd<false>>(a, s);
    if (net.general())
        return visit_cpep_general(net, hipErrorInvalidValue, [&](auto sh, auto act) {
            return launch_cpep_tan<CpepNetG<sh.nin, sh.width, sh.depth, act.hact, act.oact>>(a, s);
        });
    return visit_cpep_shapes(net, hipErrorInvalidValue, [&](auto sh) { return launch_cpep_tan<Mlp<sh.nin, sh.width, sh.depth, 1>>(a, s); });
}

#elif CUDE_SENS_PART == 2
// ---------------------------------------------------------------------------------- suppression model, fixed step
template <int W, int D, int HA, int OA>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2))) void supp_sens_kernel(SuppSensArgs a) {
    using Net = Mlp<4, W, D, 3, false, false, HA, OA>;
    constexpr int P = Net::P;
    extern __shared__ double smem[];            // [7][4][kBlock] the sweep's stage derivatives; the reduction's rows afterwards
    const int lane = threadIdx.x;
    const int64_t gid = (int64_t)blockIdx.x * kBlock + lane;
    const bool active = gid < a.N;
    const int64_t i = active ? gid : a.N - 1;
    const int T = a.T;

    const SuppTanConst k = supp_tan_load<Net>(a, i);
    const TanSums r = supp_tan_sweep<Net>(a, k, i, lane, a.cond[i], smem, [&](int oi, double d2, double d3) {
        if (a.out.sens != nullptr && active) {
            double* tr = a.out.sens + (int64_t)3 * (oi + (int64_t)T * i);
            tr[0] = 0.0;
            tr[1] = d2;
            tr[2] = d3;
        }
    });
    const bool failed = !(fabs(r.sse) <= 1.79769313486231570815e308);
    if (active) sens_finish<3>(a, i, failed, r.sse, r.info, r.score);
    const double v2[2] = {active ? r.sse : 0.0, (active && failed) ? 1.0 : 0.0};
    block_reduce_store<2>(v2, smem, a.partials + (int64_t)blockIdx.x * (P + 2) + P, lane);
}

template <int W, int D, int HA = kActHiddenTanh, int OA = kActOutSoftplus>
static hipError_t launch_supp_fixed(const SuppSensArgs& a, hipStream_t s) {
    const int64_t nblocks = (a.N + kBlock - 1) / kBlock;
    hipLaunchKernelGGL((supp_sens_kernel<W, D, HA, OA>), dim3((unsigned)nblocks), dim3(kBlock),
                       sizeof(double) * (size_t)(7 * 4) * kBlock, s, a);
    return hipGetLastError();
}

hipError_t launch_supp_sens_fixed(const NetShape& net, const SuppSensArgs& a, hipStream_t s) {
    if (a.rho == nullptr || a.obs_rho == nullptr || a.S < 1) return hipErrorInvalidValue;
    if (net.general())
        return visit_supp_general(net, hipErrorInvalidValue, [&](auto sh, auto act) {
            return launch_supp_fixed<sh.width, sh.depth, act.hact, act.oact>(a, s);
        });
    return visit_supp_shapes(net, hipErrorInvalidValue, [&](auto sh) { return launch_supp_fixed<sh.width, sh.depth>(a, s); });
}

#else
// ---------------------------------------------------------------------------------- suppression model, adaptive
template <class M>
static hipError_t launch_supp_tan(const SuppSensArgs& a, hipStream_t s) {
    const int64_t nblocks = (a.N + kBlock - 1) / kBlock;
    const size_t lds = sizeof(double) * (size_t)adaptive_rows<M>(false) * kBlock;
    hipLaunchKernelGGL((adaptive_kernel<M, false, false>), dim3((unsigned)nblocks), dim3(kBlock), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_supp_sens_adaptive(const NetShape& net, const SuppSensArgs& a, hipStream_t s) {
    if (net.general())
        return visit_supp_general(net, hipErrorInvalidValue, [&](auto sh, auto act) {
            return launch_supp_tan<SuppAdTan<sh.width, sh.depth, act.hact, act.oact>>(a, s);
        });
    return visit_supp_shapes(net, hipErrorInvalidValue, [&](auto sh) { return launch_supp_tan<SuppAdTan<sh.width, sh.depth>>(a, s); });
}
#endif

}  // namespace cude
