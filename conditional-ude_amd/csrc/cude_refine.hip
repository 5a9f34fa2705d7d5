// Newton-type per-subject fits of the conditional parameter for gfx950 (cude_refine_conditional): every subject minimises
//   F(x) = SSE_i(x) + pw (x - pc)^2   over [lower, upper]
// from its own start by a damped secant / Gauss-Newton iteration whose evaluations are tangent-linear solves.
//
// Replaces (reference repo paths) the LOCAL solver behind every per-subject fit of the reference --
//   `LBFGS` inside `Fminbox` from `initial_beta`, under ForwardDiff     src/parameter-estimation.jl:272-307, :406-433
//   validate_suppression_model                                           suppression/src/suppression_model.jl:179-222
//   the (k, sigma) fits of the symbolic model                            c-peptide/03-symreg.jl:94-106
//   compute_individual_maps (start = the current individual parameters)  src/saem.jl:74-84
// next to the global search of cude_fit_conditional (cude_common.hip fit_*), which needs no start and no derivative.
//
// Two forms of one rule (refine_update below; the rule's text is in include/cude.h):
//   * fused (fixed-step mode): one lane = one subject, one wave per workgroup; the lane keeps its subject's constants and
//     the search state in registers, every evaluation is one call of the sweep the sensitivity kernels call
//     (cude_tangent.h cpep_tan_sweep / supp_tan_sweep, here without the trajectory stores) at the trial point, and the
//     outer loop leaves when no lane of the wave is still running (ballot).  Lanes that have
//     stopped run along masked: refine_update returns at once for them, their state stays what it was.  (The host adds
//     one forward launch at the returned points, whose SSE is the one reported: cude_launch.hip.)  A second family of
//     these kernels carries a replicate dimension in the grid's y (RefineReps; cude_bootstrap_conditional): the same
//     loads, sweep and rule on observations read from a replicate slab.
//   * stepped (adaptive mode, or option "refine_fused" = 0): per evaluation one launch of the tangent solve at the trial
//     points (launch_cpep_sens / launch_supp_sens) and one refine_step_kernel; the state lives in device arrays.
//
// The file is compiled in parts (-DCUDE_REFINE_PART=k, as cude_sens.hip): 0 = the update kernel, the dispatchers, c-peptide
// shape group 0 and the symbolic model; 1 = c-peptide group 1 and the general-activation shapes; 2 = c-peptide group 2;
// 3 = the suppression model.
#include "cude_tangent.h"

namespace cude {

#ifndef CUDE_REFINE_PART
#define CUDE_REFINE_PART 0
#endif

hipError_t launch_cpep_refine_part1(const NetShape& net, int n_state, const CpepArgs& a, const RefineCfg& k, const RefineArrays& r, hipStream_t s, const RefineReps* reps);
hipError_t launch_cpep_refine_part2(const NetShape& net, int n_state, const CpepArgs& a, const RefineCfg& k, const RefineArrays& r, hipStream_t s, const RefineReps* reps);

constexpr int kRefConverged = 0, kRefAtBound = 1, kRefMaxEvals = 2, kRefFlat = 3, kRefFailed = 4;   // CUDE_REFINE_*
constexpr double kRefLambda0 = 1e-3, kRefLambdaMin = 1e-12;

// a subject's search state (registers in the fused kernels, one load / store per round in the stepped form)
struct RefineLane {
    double x, F, sse, info, g, lam, xp, gp, xt;
    int evals, status;
};

__device__ __forceinline__ bool ref_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }
__device__ __forceinline__ double ref_clamp(double v, double lo, double hi) { return v != v ? v : fmin(fmax(v, lo), hi); }

__device__ __forceinline__ void refine_start(RefineLane& s, const RefineCfg& k, double x0, bool active) {
    const double nan = __builtin_nan("");
    s.xt = ref_clamp(x0, k.lower, k.upper);
    s.x = s.xt;
    s.F = __builtin_inf();
    s.sse = s.info = s.g = nan;
    s.lam = kRefLambda0;
    s.xp = s.gp = nan;
    s.evals = 0;
    s.status = active ? kRefineRunning : kRefConverged;
}

// Steps 1-6 of the rule, entered behind the evaluation (sse_t, score_t, info_t) at s.xt: judges that trial (evals == 0: it
// is the start itself), then either stops the subject or leaves the next trial in s.xt.  The ONE statement of the rule on
// the device: both forms call it.
__device__ __forceinline__ void refine_update(RefineLane& s, const RefineCfg& k, double sse_t, double score_t, double info_t) {
    if (s.status != kRefineRunning) return;
    const double xt = s.xt;
    const double dx = xt - k.pc;
    const double Ft = sse_t + k.pw * dx * dx;
    const double gt = score_t + k.pw * dx;
    const bool fin = ref_finite(Ft);
    if (s.evals == 0) {                                       // 1
        s.sse = sse_t; s.info = info_t; s.g = gt;
        s.evals = 1;
        if (!fin) { s.status = kRefFailed; return; }
        s.F = Ft;
    } else {                                                  // 5
        s.evals++;
        if (fin && Ft < s.F) {
            s.xp = s.x; s.gp = s.g;
            s.x = xt; s.F = Ft; s.sse = sse_t; s.info = info_t; s.g = gt;
            s.lam = fmax(s.lam / 10.0, kRefLambdaMin);
        } else {
            if (fin) { s.xp = xt; s.gp = gt; }
            s.lam = s.lam * 10.0;
        }
    }
    if (s.evals >= k.max_evals) { s.status = kRefMaxEvals; return; }      // 6
    const double cs = (s.g - s.gp) / (s.x - s.xp);            // 2 (NaN while the pair is unset)
    const double H = (ref_finite(cs) && cs > 0.0) ? cs : s.info + k.pw;
    if (!(H > 0.0)) { s.status = kRefFlat; return; }
    const double d = fmin(fmax(-s.g / (H * (1.0 + s.lam)), -k.max_step), k.max_step);      // 3
    const double xn = fmin(fmax(s.x + d, k.lower), k.upper);
    if (fabs(xn - s.x) <= k.xtol * (1.0 + fabs(s.x))) {       // 4
        s.status = (xn == k.lower || xn == k.upper) ? kRefAtBound : kRefConverged;
        return;
    }
    s.xt = xn;
}

__device__ __forceinline__ void refine_store(const RefineArrays& r, int64_t i, const RefineLane& s) {
    r.x[i] = s.x;
    r.F[i] = s.F;
    r.sse[i] = s.sse;
    r.info[i] = s.info;
    r.evals[i] = s.evals;
    r.status[i] = s.status == kRefineRunning ? kRefMaxEvals : s.status;
}

// a replicate's fit (RefineReps): the point and the status alone, at q = replicate * rep_stride + subject
__device__ __forceinline__ void refine_store_rep(const RefineArrays& r, int64_t q, const RefineLane& s) {
    r.x[q] = s.x;
    r.status[q] = s.status == kRefineRunning ? kRefMaxEvals : s.status;
}

#if CUDE_REFINE_PART != 3
// ---------------------------------------------------------------------------------- c-peptide models, fused
// Net: Mlp<NIN, W, D, 1, false, false, HA, OA> or MmProd<RAW>.  The quadrature state of n_state = 3 enters no residual and
// nothing here returns it: one kernel serves either n_state.
template <class Net>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2))) void cpep_refine_kernel(CpepArgs a, RefineCfg k, RefineArrays r) {
    extern __shared__ double smem[];            // [5][2][kBlock] the sweep's stage forcings and their tangents
    const int lane = threadIdx.x;
    const int64_t gid = (int64_t)blockIdx.x * kBlock + lane;
    const bool active = gid < a.N;
    const int64_t i = active ? gid : a.N - 1;

    const CpepTanConst kc = cpep_tan_load<Net>(a, i);
    RefineLane st;
    refine_start(st, k, r.x0[i], active);
#pragma unroll 1
    while (__ballot(st.status == kRefineRunning) != 0ull) {
        const TanSums e = cpep_tan_sweep<Net, 2>(a, kc, i, lane, st.xt, smem, TanNoStore());
        refine_update(st, k, e.sse, e.score + e.chk, e.info + e.chk);
    }
    if (active) refine_store(r, i, st);
}

// ... with a replicate dimension (RefineReps): the kernel's own copy of the argument block gets its observations pointed at the
// replicate's, the sweep and the rule are the calls above
template <class Net>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2))) void cpep_refine_reps_kernel(CpepArgs a, RefineCfg k, RefineArrays r,
                                                                                                          RefineReps p) {
    extern __shared__ double smem[];
    const int lane = threadIdx.x;
    const int64_t gid = ((int64_t)blockIdx.x + p.blk_first) * kBlock + lane;
    const bool active = gid < a.N;
    const int64_t i = active ? gid : a.N - 1;
    a.obs = p.slab + (int64_t)blockIdx.y * p.slab_stride;

    const CpepTanConst kc = cpep_tan_load<Net>(a, i);
    RefineLane st;
    refine_start(st, k, r.x0[i], active);
#pragma unroll 1
    while (__ballot(st.status == kRefineRunning) != 0ull) {
        const TanSums e = cpep_tan_sweep<Net, 2>(a, kc, i, lane, st.xt, smem, TanNoStore());
        refine_update(st, k, e.sse, e.score + e.chk, e.info + e.chk);
    }
    if (active) refine_store_rep(r, (int64_t)blockIdx.y * p.rep_stride + i, st);
}

template <class Net>
static hipError_t launch_cpep_fused(int n_state, const CpepArgs& a, const RefineCfg& k, const RefineArrays& r, hipStream_t s, const RefineReps* reps) {
    const int64_t nblocks = (a.N + kBlock - 1) / kBlock;
    const size_t lds = sizeof(double) * (size_t)10 * kBlock;
    if (reps != nullptr) {
        hipLaunchKernelGGL((cpep_refine_reps_kernel<Net>), dim3((unsigned)reps->blk_count, (unsigned)reps->n_reps), dim3(kBlock), lds, s, a,
                           k, r, *reps);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((cpep_refine_kernel<Net>), dim3((unsigned)nblocks), dim3(kBlock), lds, s, a, k, r);
    return hipGetLastError();
}
#endif

#if CUDE_REFINE_PART == 0
// ---------------------------------------------------------------------------------- stepped form: the update kernel
__global__ __launch_bounds__(256) void refine_step_kernel(int phase, RefineCfg k, RefineArrays r) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= r.N) return;
    RefineLane s;
    if (phase == 2) {                                         // objective from the SSE cude_forward's kernel left in r.sse
        if (r.status[i] == kRefFailed) return;
        const double dx = r.x[i] - k.pc;
        r.F[i] = r.sse[i] + k.pw * dx * dx;
        return;
    }
    if (phase == 0) {
        refine_start(s, k, r.x0[i], true);
    } else {
        s.status = r.status[i];
        if (s.status != kRefineRunning) return;               // a stopped subject keeps its state bit for bit
        s.x = r.x[i]; s.F = r.F[i]; s.sse = r.sse[i]; s.info = r.info[i]; s.g = r.g[i];
        s.lam = r.lam[i]; s.xp = r.xp[i]; s.gp = r.gp[i]; s.xt = r.xt[i];
        s.evals = r.evals[i];
        refine_update(s, k, r.sse_t[i], r.score_t[i], r.info_t[i]);
    }
    r.x[i] = s.x; r.F[i] = s.F; r.sse[i] = s.sse; r.info[i] = s.info; r.g[i] = s.g;
    r.lam[i] = s.lam; r.xp[i] = s.xp; r.gp[i] = s.gp; r.xt[i] = s.xt;
    r.evals[i] = s.evals; r.status[i] = s.status;
}

hipError_t launch_refine_step(int phase, const RefineCfg& k, const RefineArrays& r, hipStream_t s) {
    hipLaunchKernelGGL(refine_step_kernel, dim3((unsigned)((r.N + 255) / 256)), dim3(256), 0, s, phase, k, r);
    return hipGetLastError();
}

hipError_t launch_cpep_refine(const NetShape& net, int n_state, const CpepArgs& a, const RefineCfg& k, const RefineArrays& r, hipStream_t s, const RefineReps* reps) {
    if (net.generic() || a.obs == nullptr || a.T < 1 || a.S < 1 || (n_state != 2 && n_state != 3)) return hipErrorInvalidValue;
    if (net.symbolic())
        return a.cond_raw ? launch_cpep_fused<MmProd<true>>(n_state, a, k, r, s, reps) : launch_cpep_fused<MmProd<false>>(n_state, a, k, r, s, reps);
    if (net.general()) return launch_cpep_refine_part1(net, n_state, a, k, r, s, reps);
    hipError_t e = visit_cpep_shapes_0(net, hipErrorNotSupported, [&](auto sh) {
        return launch_cpep_fused<Mlp<sh.nin, sh.width, sh.depth, 1>>(n_state, a, k, r, s, reps);
    });
    if (e == hipErrorNotSupported) e = launch_cpep_refine_part1(net, n_state, a, k, r, s, reps);
    return e != hipErrorNotSupported ? e : launch_cpep_refine_part2(net, n_state, a, k, r, s, reps);
}

#elif CUDE_REFINE_PART == 1
// hipErrorNotSupported = not in this group
hipError_t launch_cpep_refine_part1(const NetShape& net, int n_state, const CpepArgs& a, const RefineCfg& k, const RefineArrays& r, hipStream_t s, const RefineReps* reps) {
    if (net.general())
        return visit_cpep_general(net, hipErrorInvalidValue, [&](auto sh, auto act) {
            return launch_cpep_fused<CpepNetG<sh.nin, sh.width, sh.depth, act.hact, act.oact>>(n_state, a, k, r, s, reps);
        });
    return visit_cpep_shapes_1(net, hipErrorNotSupported, [&](auto sh) {
        return launch_cpep_fused<Mlp<sh.nin, sh.width, sh.depth, 1>>(n_state, a, k, r, s, reps);
    });
}

#elif CUDE_REFINE_PART == 2
hipError_t launch_cpep_refine_part2(const NetShape& net, int n_state, const CpepArgs& a, const RefineCfg& k, const RefineArrays& r, hipStream_t s, const RefineReps* reps) {
    return visit_cpep_shapes_2(net, hipErrorInvalidValue, [&](auto sh) {
        return launch_cpep_fused<Mlp<sh.nin, sh.width, sh.depth, 1>>(n_state, a, k, r, s, reps);
    });
}

#else
// ---------------------------------------------------------------------------------- suppression model, fused
template <int W, int D, int HA, int OA>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2))) void supp_refine_kernel(SuppArgs a, RefineCfg k, RefineArrays r) {
    using Net = Mlp<4, W, D, 3, false, false, HA, OA>;
    extern __shared__ double smem[];            // [7][4][kBlock] the sweep's stage derivatives
    const int lane = threadIdx.x;
    const int64_t gid = (int64_t)blockIdx.x * kBlock + lane;
    const bool active = gid < a.N;
    const int64_t i = active ? gid : a.N - 1;

    const SuppTanConst kc = supp_tan_load<Net>(a, i);
    RefineLane rs;
    refine_start(rs, k, r.x0[i], active);
#pragma unroll 1
    while (__ballot(rs.status == kRefineRunning) != 0ull) {
        const TanSums e = supp_tan_sweep<Net>(a, kc, i, lane, rs.xt, smem, TanNoStore());
        refine_update(rs, k, e.sse, e.score, e.info);
    }
    if (active) refine_store(r, i, rs);
}

// ... with a replicate dimension, as cpep_refine_reps_kernel
template <int W, int D, int HA, int OA>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2))) void supp_refine_reps_kernel(SuppArgs a, RefineCfg k, RefineArrays r,
                                                                                                          RefineReps p) {
    using Net = Mlp<4, W, D, 3, false, false, HA, OA>;
    extern __shared__ double smem[];
    const int lane = threadIdx.x;
    const int64_t gid = ((int64_t)blockIdx.x + p.blk_first) * kBlock + lane;
    const bool active = gid < a.N;
    const int64_t i = active ? gid : a.N - 1;
    a.data = p.slab + (int64_t)blockIdx.y * p.slab_stride;

    const SuppTanConst kc = supp_tan_load<Net>(a, i);
    RefineLane rs;
    refine_start(rs, k, r.x0[i], active);
#pragma unroll 1
    while (__ballot(rs.status == kRefineRunning) != 0ull) {
        const TanSums e = supp_tan_sweep<Net>(a, kc, i, lane, rs.xt, smem, TanNoStore());
        refine_update(rs, k, e.sse, e.score, e.info);
    }
    if (active) refine_store_rep(r, (int64_t)blockIdx.y * p.rep_stride + i, rs);
}

template <int W, int D, int HA = kActHiddenTanh, int OA = kActOutSoftplus>
static hipError_t launch_supp_fused(const SuppArgs& a, const RefineCfg& k, const RefineArrays& r, hipStream_t s, const RefineReps* reps) {
    const int64_t nblocks = (a.N + kBlock - 1) / kBlock;
    if (reps != nullptr) {
        hipLaunchKernelGGL((supp_refine_reps_kernel<W, D, HA, OA>), dim3((unsigned)reps->blk_count, (unsigned)reps->n_reps), dim3(kBlock),
                           sizeof(double) * (size_t)(7 * 4) * kBlock, s, a, k, r, *reps);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((supp_refine_kernel<W, D, HA, OA>), dim3((unsigned)nblocks), dim3(kBlock),
                       sizeof(double) * (size_t)(7 * 4) * kBlock, s, a, k, r);
    return hipGetLastError();
}

hipError_t launch_supp_refine(const NetShape& net, const SuppArgs& a, const RefineCfg& k, const RefineArrays& r, hipStream_t s, const RefineReps* reps) {
    if (net.nin != 4 || net.generic() || a.T < 1 || a.T_data > 0 || a.rho == nullptr || a.obs_rho == nullptr || a.S < 1)
        return hipErrorInvalidValue;
    if (net.general())
        return visit_supp_general(net, hipErrorInvalidValue, [&](auto sh, auto act) {
            return launch_supp_fused<sh.width, sh.depth, act.hact, act.oact>(a, k, r, s, reps);
        });
    return visit_supp_shapes(net, hipErrorInvalidValue, [&](auto sh) { return launch_supp_fused<sh.width, sh.depth>(a, k, r, s, reps); });
}
#endif

}  // namespace cude
