// Posterior-predictive bands (cude_predictive_bands, include/cude.h): exact order statistics and the sequential mean of the
// n_sets sample trajectories of every (subject, output time) column, taken where the multi-set dense-output solve left them.
//
// Replaces (reference repo paths): the loop that simulates every thinned posterior sample of an individual and summarises
// the curves, c-peptide/06-saem.jl:209-241 (the solves themselves: src/saem.jl:31-53, run by the dense-output kernels).
//
// Input: the slab of one solve launch -- stride 1 in the state, then output time, then subject, the set slowest -- so the K
// values of one column lie a whole set apart while neighbouring columns of one set are col_stride (= n_state) doubles
// apart.  A workgroup therefore takes a TILE of C neighbouring columns: the read of one set is one contiguous stretch of
// C * n_state * 8 bytes (a lone column would use 8 bytes of every cache line it touches).
//
// LDS: the tile as [Kp][C] doubles, Kp = K rounded up to a power of two and padded with +Inf, element e of column c at
// e * C + c (neighbouring lanes = neighbouring columns or neighbouring elements: 8-byte accesses without bank conflicts
// once C * j >= 32).  C = min(64, 8192 / Kp): at most 64 KiB per workgroup, i.e. two workgroups (8 waves) per compute unit
// of 160 KiB at every K, more when the tile is smaller than 64 KiB (K <= 64).
//
// Per workgroup: load; one lane per column walks its K values IN SET ORDER (the mean's plain adds, the finiteness test, the
// per-set flags); a bitonic sorting network over all C columns at once (each compare-exchange stays inside its column);
// the wanted ranks are read off.  Sorting is a permutation, so every output is one of the solve's own values.
#include <hip/hip_runtime.h>

#include "cude_kernels.h"
#include "cude_observe.h"
#include "cude_tilesort.h"

namespace cude {

namespace {
constexpr int kPredThreads = kTileSortThreads;
constexpr int kPredMaxCols = kTileSortMaxCols;

__global__ __launch_bounds__(kPredThreads) void predictive_select_kernel(PredictiveArgs a, const int32_t* __restrict__ ranks,
                                                                         int lgC, int Kp) {
    extern __shared__ double s_v[];                 // [Kp][C]
    __shared__ int32_t s_bad[kPredMaxCols];
    const int tid = threadIdx.x;
    const int C = 1 << lgC;
    const int64_t q0 = (int64_t)blockIdx.x * C;     // first column of the tile
    const int n_el = Kp << lgC;
    const double inf = __builtin_huge_val();
    // (tile_fill's loop, kept here in its own words: through tile_fill this kernel compiles to one scalar move more than
    // before, profiles/replicates_split.txt)
    for (int idx = tid; idx < n_el; idx += kPredThreads) {
        const int cc = idx & (C - 1), k = idx >> lgC;
        const int64_t q = q0 + cc;
        s_v[idx] = (k < a.K && q < a.n_cols) ? a.slab[(int64_t)k * a.set_stride + q * a.col_stride] : inf;
    }
    __syncthreads();
    // ---- one lane per column, in set order: rule 3's sum, rule 4's test
    if (tid < C) {
        const int64_t q = q0 + tid;
        bool bad = false;
        if (q < a.n_cols) {
            const int64_t subj = a.subj0 + q / a.Tc;
            uint8_t* const flag = a.bad + subj * a.bad_stride;
            double acc = s_v[tid];
            if (!finite_value(acc)) { bad = true; flag[0] = 1; }
#pragma unroll 8
            for (int k = 1; k < a.K; k++) {
                const double v = s_v[(k << lgC) + tid];
                acc = acc + v;
                if (!finite_value(v)) { bad = true; flag[k] = 1; }
            }
            if (a.mean != nullptr)
                a.mean[a.t0 + q % a.Tc + (int64_t)a.n_times * subj] = bad ? __builtin_nan("") : acc / (double)a.K;
        }
        s_bad[tid] = bad ? 1 : 0;
    }
    if (a.n_ranks == 0) return;
    tile_sort_ascending(s_v, lgC, Kp, tid);      // (cude_tilesort.h)
    for (int idx = tid; idx < a.n_ranks << lgC; idx += kPredThreads) {
        const int r = idx % a.n_ranks, cc = idx / a.n_ranks;
        const int64_t q = q0 + cc;
        if (q >= a.n_cols) continue;
        const int64_t subj = a.subj0 + q / a.Tc;
        const int64_t col = a.t0 + q % a.Tc + (int64_t)a.n_times * subj;
        a.order[r + (int64_t)a.n_ranks * col] = s_bad[cc] ? __builtin_nan("") : s_v[(ranks[r] << lgC) + cc];
    }
}

__global__ void predictive_count_kernel(int64_t N, int K, const uint8_t* __restrict__ bad, int32_t* __restrict__ bad_sets) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    int32_t n = 0;
    for (int k = 0; k < K; k++) n += bad[i * K + k];
    bad_sets[i] = n;
}
}  // namespace

// ranks_dev: [n_ranks] on the device, validated by the caller
hipError_t launch_predictive_select(const PredictiveArgs& a, const int32_t* ranks_dev, hipStream_t s) {
    if (a.K < 1 || a.K > kPredMaxSets || a.n_ranks < 0 || a.n_ranks > kPredMaxRanks || a.n_cols < 1 || a.Tc < 1)
        return hipErrorInvalidValue;
    return tile_launch(predictive_select_kernel, tile_geometry(a.K), a.n_cols, s, a, ranks_dev);
}

hipError_t launch_predictive_count(int64_t N, int K, const uint8_t* bad, int32_t* bad_sets, hipStream_t s) {
    const int bs = 256;
    hipLaunchKernelGGL(predictive_count_kernel, dim3((unsigned)((N + bs - 1) / bs)), dim3(bs), 0, s, N, K, bad, bad_sets);
    return hipGetLastError();
}

}  // namespace cude
