// Order-2 forward-mode ensemble solves for gfx950: every subject's trajectory together with its first AND second derivative
// with respect to the subject's own conditional parameter (cude_curvature), hence the exact curvature of its objective,
//   (1/2) d^2 SSE_i / d cond_i^2 = sum w^2 [(d yhat / d cond)^2 + (yhat - y) d^2 yhat / d cond^2] = info_i + curv2_i,
// where cude_sensitivity gives the Gauss-Newton term info_i alone.
//
// Replaces (reference repo paths): what ForwardDiff.hessian / nested duals through `solve` would give for the per-subject
// objective of src/parameter-estimation.jl:165,370 and suppression/src/suppression_model.jl:155 in the direction
// d/d(beta_i) resp. d/d(theta_i) -- observed-information standard errors, the Laplace approximation of a subject's
// marginal likelihood, and the sign test that tells a conditional minimum from a saddle.
//
// The structure is cude_sens.hip's, one Taylor coefficient further: one lane = one subject, no reduction over subjects
// except the (sum SSE, failures) pair; the fixed-step sweeps are in cude_tangent2.h (cpep_tan2_sweep / supp_tan2_sweep),
// the adaptive solves are the order-2 policies (CpepAdCurv / SuppAdCurv, cude_adaptive.h) over the one-body kernel.  The
// network is evaluated by Mlp::eval_jet2 / MmProd::eval_jet2 (cude_device.h): every weight column is read once for the
// value and both derivatives.  Failure convention: cude_sensitivity's.
//
// The file is compiled in parts (-DCUDE_CURV_PART=k, as cude_sens.hip): 0 = c-peptide fixed-step + the dispatchers,
// 1 = c-peptide adaptive, 2 = suppression fixed-step, 3 = suppression adaptive.
#include "cude_adaptive_body.h"
#include "cude_tangent2.h"

namespace cude {

#ifndef CUDE_CURV_PART
#define CUDE_CURV_PART 0
#endif

hipError_t launch_cpep_curv_adaptive(const NetShape& net, const CpepCurvArgs& a, hipStream_t s);
hipError_t launch_supp_curv_fixed(const NetShape& net, const SuppCurvArgs& a, hipStream_t s);
hipError_t launch_supp_curv_adaptive(const NetShape& net, const SuppCurvArgs& a, hipStream_t s);

// per-subject outputs behind a fixed-step solve (bad: NaN throughout)
template <int NS, class Args>
__device__ __forceinline__ void curv_finish(const Args& a, int64_t i, bool bad, const TanSums2& r) {
    const double nan = __builtin_nan("");
    if (a.sse != nullptr) a.sse[i] = r.sse;
    if (a.out.info != nullptr) a.out.info[i] = bad ? nan : r.info;
    if (a.out.score != nullptr) a.out.score[i] = bad ? nan : r.score;
    if (a.out2.curv != nullptr) a.out2.curv[i] = bad ? nan : r.info + r.curv2;
    if (bad && a.out2.sens2 != nullptr)
        for (int q = 0; q < NS * a.T; q++) a.out2.sens2[(int64_t)NS * a.T * i + q] = nan;
}

#if CUDE_CURV_PART == 0
// ---------------------------------------------------------------------------------- c-peptide models, fixed step
// Net: Mlp<NIN, W, D, 1, false, false, HA, OA> or MmProd<RAW>.  NS = 3: + the cumulative-secretion quadrature state.
template <class Net, int NS>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2))) void cpep_curv_kernel(CpepCurvArgs a) {
    constexpr int P = Net::P;
    extern __shared__ double smem[];
    double* s_q = smem;                         // [5][3][kBlock] stage forcings, their first and second derivatives
    double* s_red = smem + 15 * kBlock;         // [kRedRows][kBlock]
    const int lane = threadIdx.x;
    const int64_t gid = (int64_t)blockIdx.x * kBlock + lane;
    const bool active = gid < a.N;
    const int64_t i = active ? gid : a.N - 1;
    const int T = a.T;

    const CpepTanConst k = cpep_tan_load<Net>(a, i);
    const TanSums2 r = cpep_tan2_sweep<Net, NS>(a, k, i, lane, a.cond[i], s_q, [&](int oi, double e1, double e2, double e3) {
        if (a.out2.sens2 != nullptr && active) {
            double* tr = a.out2.sens2 + (int64_t)NS * (oi + (int64_t)T * i);
            tr[0] = e1;
            tr[1] = e2;
            if (NS == 3) tr[2] = e3;
        }
    });
    const bool failed = !(fabs(r.sse) <= 1.79769313486231570815e308);   // NaN or Inf
    if (active) curv_finish<NS>(a, i, failed, r);
    const double v2[2] = {active ? r.sse : 0.0, (active && failed) ? 1.0 : 0.0};
    block_reduce_store<2>(v2, s_red, a.partials + (int64_t)blockIdx.x * (P + 2) + P, lane);
}

template <class Net>
static hipError_t launch_cpep_fixed(int n_state, const CpepCurvArgs& a, hipStream_t s) {
    const int64_t nblocks = (a.N + kBlock - 1) / kBlock;
    const size_t lds = sizeof(double) * (size_t)(15 + kRedRows) * kBlock;
    if (n_state == 2) hipLaunchKernelGGL((cpep_curv_kernel<Net, 2>), dim3((unsigned)nblocks), dim3(kBlock), lds, s, a);
    else hipLaunchKernelGGL((cpep_curv_kernel<Net, 3>), dim3((unsigned)nblocks), dim3(kBlock), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_cpep_curv(const NetShape& net, int n_state, const CpepCurvArgs& a, hipStream_t s) {
    if (net.generic() || a.partials == nullptr || a.obs == nullptr || a.T < 1 || a.n_sets > 1) return hipErrorInvalidValue;
    if (a.S == 0) return n_state == 2 ? launch_cpep_curv_adaptive(net, a, s) : hipErrorInvalidValue;
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

hipError_t launch_supp_curv(const NetShape& net, const SuppCurvArgs& a, hipStream_t s) {
    if (net.nin != 4 || net.generic() || a.partials == nullptr || a.T < 1 || a.n_sets > 1 || a.T_data > 0) return hipErrorInvalidValue;
    return a.S == 0 ? launch_supp_curv_adaptive(net, a, s) : launch_supp_curv_fixed(net, a, s);
}

#elif CUDE_CURV_PART == 1
// ---------------------------------------------------------------------------------- c-peptide models, adaptive
template <class Net>
static hipError_t launch_cpep_jet(const CpepCurvArgs& a, hipStream_t s) {
    using M = CpepAdCurv<Net>;
    const int64_t nblocks = (a.N + kBlock - 1) / kBlock;
    const size_t lds = sizeof(double) * (size_t)(adaptive_rows<M>(false) + a.TG) * kBlock;
    hipLaunchKernelGGL((adaptive_kernel<M, true, false>), dim3((unsigned)nblocks), dim3(kBlock), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_cpep_curv_adaptive(const NetShape& net, const CpepCurvArgs& a, hipStream_t s) {
    if (a.TG < 2 || a.TG > kMaxObs) return hipErrorInvalidValue;
    if (net.symbolic()) return a.cond_raw ? launch_cpep_jet<MmProd<true>>(a, s) : launch_cpep_jet<MmProd<false>>(a, s);
    // (the general-activation shapes: fixed-step mode only)
    if (net.general()) return hipErrorInvalidValue;
    return visit_cpep_shapes(net, hipErrorInvalidValue, [&](auto sh) { return launch_cpep_jet<Mlp<sh.nin, sh.width, sh.depth, 1>>(a, s); });
}

#elif CUDE_CURV_PART == 2
// ---------------------------------------------------------------------------------- suppression model, fixed step
template <int W, int D, int HA, int OA>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2))) void supp_curv_kernel(SuppCurvArgs a) {
    using Net = Mlp<4, W, D, 3, false, false, HA, OA>;
    constexpr int P = Net::P;
    extern __shared__ double smem[];            // [7][6][kBlock] the sweep's stage derivatives; the reduction's rows afterwards
    const int lane = threadIdx.x;
    const int64_t gid = (int64_t)blockIdx.x * kBlock + lane;
    const bool active = gid < a.N;
    const int64_t i = active ? gid : a.N - 1;
    const int T = a.T;

    const SuppTanConst k = supp_tan_load<Net>(a, i);
    const TanSums2 r = supp_tan2_sweep<Net>(a, k, i, lane, a.cond[i], smem, [&](int oi, double e2, double e3) {
        if (a.out2.sens2 != nullptr && active) {
            double* tr = a.out2.sens2 + (int64_t)3 * (oi + (int64_t)T * i);
            tr[0] = 0.0;
            tr[1] = e2;
            tr[2] = e3;
        }
    });
    const bool failed = !(fabs(r.sse) <= 1.79769313486231570815e308);
    if (active) curv_finish<3>(a, i, failed, r);
    const double v2[2] = {active ? r.sse : 0.0, (active && failed) ? 1.0 : 0.0};
    __syncthreads();                            // (no lane's stage rows are read after this point; the rows are per lane)
    block_reduce_store<2>(v2, smem, a.partials + (int64_t)blockIdx.x * (P + 2) + P, lane);
}

template <int W, int D, int HA = kActHiddenTanh, int OA = kActOutSoftplus>
static hipError_t launch_supp_fixed(const SuppCurvArgs& a, hipStream_t s) {
    const int64_t nblocks = (a.N + kBlock - 1) / kBlock;
    static_assert(7 * 6 >= kRedRows, "the reduction's rows alias the stage rows");
    hipLaunchKernelGGL((supp_curv_kernel<W, D, HA, OA>), dim3((unsigned)nblocks), dim3(kBlock),
                       sizeof(double) * (size_t)(7 * 6) * kBlock, s, a);
    return hipGetLastError();
}

hipError_t launch_supp_curv_fixed(const NetShape& net, const SuppCurvArgs& a, hipStream_t s) {
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
static hipError_t launch_supp_jet(const SuppCurvArgs& a, hipStream_t s) {
    const int64_t nblocks = (a.N + kBlock - 1) / kBlock;
    const size_t lds = sizeof(double) * (size_t)adaptive_rows<M>(false) * kBlock;
    hipLaunchKernelGGL((adaptive_kernel<M, false, false>), dim3((unsigned)nblocks), dim3(kBlock), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_supp_curv_adaptive(const NetShape& net, const SuppCurvArgs& a, hipStream_t s) {
    // (the general-activation shapes: fixed-step mode only)
    if (net.general()) return hipErrorInvalidValue;
    return visit_supp_shapes(net, hipErrorInvalidValue, [&](auto sh) { return launch_supp_jet<SuppAdCurv<sh.width, sh.depth>>(a, s); });
}
#endif

}  // namespace cude
