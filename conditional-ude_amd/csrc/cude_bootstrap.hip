// Parametric bootstrap of the per-subject conditional fits (cude_bootstrap_conditional, include/cude.h): the kernels around
// the replicate launch of the fused refinement (cude_refine.hip, RefineReps).
//
// Replaces (reference repo paths) the loop a caller of the reference writes to see the finite-sample spread of an estimate --
// simulate noisy data from the fitted model, fit it again: suppression/src/suppression_model.jl:39-63 (the noisy data),
// :179-222 (the per-subject refit).
//
//   * bootstrap_generate_kernel: the replicate observations, in the population's own layout so that the sweeps of
//     cude_tangent.h read them through the pointer they always read ([rows][N] per replicate, the replicate slowest).  One
//     thread per (subject, row, replicate); neighbouring threads = neighbouring subjects: every access is contiguous.  Each
//     operation of  yhat + (sigma s) eps  is rounded on its own, so a caller can rebuild a replicate's data to the bit.
//   * bootstrap_reduce_kernel: rule 5.  A workgroup takes a tile of C neighbouring subjects and all K replicates into LDS
//     ([Kp][C], the estimates of FAILED replicates as +Inf -- an estimate that did not fail lies inside the box); one lane per
//     subject walks its column in replicate order (count, plain sum, second pass for the sd); the tile is sorted by the
//     network cude_predictive.hip sorts with (cude_tilesort.h), +Inf last, and the ranks below n_used are read off.
#include "cude_kernels.h"
#include "cude_observe.h"
#include "cude_rng.h"
#include "cude_tilesort.h"

namespace cude {

namespace {
constexpr int kGenThreads = 256;
constexpr int kRefFailedStatus = 4;               // CUDE_REFINE_FAILED

// rule 5's second pass, every operation rounded on its own (as rule 2's, cude_observe.h): ss + (v - mean) (v - mean)
__device__ __forceinline__ double bootstrap_square_add(double ss, double v, double mean) {
#pragma clang fp contract(off)
    const double d = v - mean;
    const double q = d * d;
    return ss + q;
}

// out: the slab (noise_only = false) or the table of the draws themselves
template <bool NOISE_ONLY>
__global__ __launch_bounds__(kGenThreads) void bootstrap_generate_kernel(BootstrapGenArgs a, double* __restrict__ out) {
    const int64_t li = (int64_t)blockIdx.x * kGenThreads + threadIdx.x;
    if (li >= a.n_subj) return;
    const int64_t i = a.subj0 + li;
    const int r = blockIdx.y, b = blockIdx.z;
    const int s = r / a.T, t = r - s * a.T;
    const int64_t q = ((int64_t)b * (a.n_states * a.T) + r) * a.N + i;
    if (t == 0) {                                 // the initial state: never drawn
        out[q] = NOISE_ONLY ? 0.0 : a.pop[(int64_t)r * a.N + i];
        return;
    }
    const double eps = (!NOISE_ONLY && a.from_noise) ? out[q] : rng_bootstrap_normal(a.seed, a.subject_offset + i, a.first_rep + b, r);
    if (NOISE_ONLY) {
        out[q] = eps;
        return;
    }
    const double yhat = a.traj[s + (int64_t)a.traj_states * (t + (int64_t)a.T * i)];
    out[q] = simulated_observation(yhat, a.sigma[i], a.scale[s], eps);      // rule 2
}

__global__ __launch_bounds__(kTileSortThreads) void bootstrap_reduce_kernel(BootstrapReduceArgs a, const int32_t* __restrict__ ranks,
                                                                            int lgC, int Kp) {
    extern __shared__ double s_v[];               // [Kp][C]
    __shared__ int32_t s_n[kTileSortMaxCols];
    const int tid = threadIdx.x;
    const int C = 1 << lgC;
    const int64_t q0 = (int64_t)blockIdx.x * C;   // first subject of the tile
    const double inf = __builtin_huge_val();
    tile_fill(s_v, C, lgC, Kp, tid, [&](int k, int cc) {
        const int64_t q = q0 + cc;
        double v = inf;
        if (k < a.K && q < a.n_subj && a.status[(int64_t)k * a.stride + q] != kRefFailedStatus) v = a.reps[(int64_t)k * a.stride + q];
        return v;
    });
    __syncthreads();
    // ---- one lane per subject, in replicate order
    if (tid < C) {
        const int64_t q = q0 + tid;
        int n = 0;
        if (q < a.n_subj) {
            double sum = 0.0;
            for (int k = 0; k < a.K; k++) {
                const double v = s_v[(k << lgC) + tid];
                if (v < inf) { n++; sum = sum + v; }
            }
            const double nan = __builtin_nan("");
            const double mean = n > 0 ? sum / (double)n : nan;
            double ss = 0.0;
            for (int k = 0; k < a.K; k++) {
                const double v = s_v[(k << lgC) + tid];
                if (v < inf) ss = bootstrap_square_add(ss, v, mean);
            }
            a.n_used[q] = n;
            if (a.mean != nullptr) a.mean[q] = mean;
            if (a.sd != nullptr) a.sd[q] = n > 1 ? sqrt(ss / (double)(n - 1)) : nan;
        }
        s_n[tid] = n;
    }
    if (a.n_ranks == 0) return;
    tile_sort_ascending(s_v, lgC, Kp, tid);
    for (int idx = tid; idx < a.n_ranks << lgC; idx += kTileSortThreads) {
        const int cc = idx & (C - 1), r = idx >> lgC;
        const int64_t q = q0 + cc;
        if (q >= a.n_subj) continue;
        a.order[(int64_t)r * a.out_stride + q] = ranks[r] < s_n[cc] ? s_v[(ranks[r] << lgC) + cc] : __builtin_nan("");
    }
}

bool gen_args_ok(const BootstrapGenArgs& a) {
    return a.n_subj >= 1 && a.subj0 >= 0 && a.subj0 + a.n_subj <= a.N && a.T >= 1 && a.n_states >= 1 && a.n_states <= 3 &&
           a.n_states * a.T <= 65535 && a.n_reps >= 1 && a.n_reps <= kPredMaxSets && a.first_rep >= 0 &&
           a.first_rep + a.n_reps <= kRngMaxReplicate;
}
dim3 gen_grid(const BootstrapGenArgs& a) {
    return dim3((unsigned)((a.n_subj + kGenThreads - 1) / kGenThreads), (unsigned)(a.n_states * a.T), (unsigned)a.n_reps);
}
}  // namespace

hipError_t launch_bootstrap_generate(const BootstrapGenArgs& a, hipStream_t s) {
    if (!gen_args_ok(a) || !a.slab || !a.traj || !a.sigma || !a.pop) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bootstrap_generate_kernel<false>, gen_grid(a), dim3(kGenThreads), 0, s, a, a.slab);
    return hipGetLastError();
}

hipError_t launch_bootstrap_noise(const BootstrapGenArgs& a, double* out, hipStream_t s) {
    if (!gen_args_ok(a) || !out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bootstrap_generate_kernel<true>, gen_grid(a), dim3(kGenThreads), 0, s, a, out);
    return hipGetLastError();
}

// ranks_dev: [n_ranks] on the device, validated by the caller
hipError_t launch_bootstrap_reduce(const BootstrapReduceArgs& a, const int32_t* ranks_dev, hipStream_t s) {
    if (a.K < 1 || a.K > kPredMaxSets || a.n_ranks < 0 || a.n_subj < 1 || !a.reps || !a.status || !a.n_used ||
        (a.n_ranks > 0 && (!a.order || !ranks_dev)))
        return hipErrorInvalidValue;
    return tile_launch(bootstrap_reduce_kernel, tile_geometry(a.K), a.n_subj, s, a, ranks_dev);
}

}  // namespace cude
