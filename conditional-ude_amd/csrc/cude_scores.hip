// Per-subject network scores (cude_subject_scores; the numbered rules in include/cude.h): the gradient launches leave the
// lanes' own rows d SSE_i(x_ik) / d theta in a [set][P][N] table (CpepArgs::lane_rows), and the kernels here fold the sets
// of every subject into one weighted row, finish it (failures, parameter mask, the caller's [N][P] layout) and form the
// sum and the cross product (outer-product-of-gradients matrix) of the rows over the subjects.
//
// Fold: one lane per (parameter, subject).  A subject's sets are added strictly in set order by ONE lane into state that
// lives in device memory between the launches of a call, every product and every sum rounded on its own (contraction
// off): no output depends on how the sets were split over launches.
//
// Sum and cross product: plain FMAs, no MFMA.  cross[q][r] is a dot product of two contiguous rows of N doubles; the
// table is read once per tile row (P = 67: 5 tile rows), so the cost is that of streaming it a few times through L2 --
// 0.9 GFLOP over 54 MB at N = 1e5, P = 67 is bandwidth and latency, not arithmetic (measurements: profiles/scores.txt).
// The association order is fixed by N alone: subjects in blocks of kCrossSubjects, inside a block in index order by one
// lane per entry, the blocks' partial sums added in block order by one lane per entry.  Only the upper triangle's tiles
// are computed; the finishing kernel writes every value to both triangles.  The sum over the subjects is the cross
// product with a row of ones appended as parameter P (a product by 1.0 is exact, so the FMA is a plain addition); a
// failed subject's column is zero in every row, the ones' included.
#include <hip/hip_runtime.h>

#include "cude_kernels.h"

namespace cude {

namespace {
constexpr int kScoreThreads = 256;
constexpr int kCrossTile = 16;                    // entries of a tile: kCrossTile x kCrossTile, one lane each
constexpr int kCrossSub = 128;                    // subjects staged in LDS at a time (2 x 16 rows: 33 KB) ...
constexpr int kCrossSubjects = 1024;              // ... and per workgroup (one partial sum per entry and workgroup)
constexpr int kCrossPitch = kCrossSub + 1;        // LDS row pitch: the 16 rows a wave reads at once fall into 16 banks
constexpr double kDblMax = 1.79769313486231570815e308;

__device__ __forceinline__ bool is_finite(double v) { return fabs(v) <= kDblMax; }

// the fold's one operation: s + (w * row), the product rounded, then the sum
__device__ __forceinline__ double fold_term(double s, double w, double row) {
#pragma clang fp contract(off)
    const double p = w * row;
    return s + p;
}

// grid: x over the subjects, y over the parameters 0 ... P - 1 and, as row P, the weighted SSE with the count of bad sets
__global__ __launch_bounds__(kScoreThreads) void scores_fold_kernel(ScoresArgs a, int kn, int first,
                                                                     const double* __restrict__ rows,
                                                                     const double* __restrict__ sse,
                                                                     const double* __restrict__ w) {
    const int64_t i = (int64_t)blockIdx.x * kScoreThreads + threadIdx.x;
    if (i >= a.N) return;
    const int64_t N = a.N;
    const int P = a.P;
    const int q = blockIdx.y;
    if (q < P) {
        double s = first ? 0.0 : a.s[(int64_t)q * N + i];
        for (int k = 0; k < kn; k++) {
            const double wk = w != nullptr ? w[(int64_t)k * N + i] : 1.0;
            if (wk != 0.0) s = fold_term(s, wk, rows[((int64_t)k * P + q) * N + i]);
        }
        a.s[(int64_t)q * N + i] = s;
        return;
    }
    double ws = first ? 0.0 : a.wsse[i];
    int32_t nb = first ? 0 : a.bad[i];
    for (int k = 0; k < kn; k++) {
        const double wk = w != nullptr ? w[(int64_t)k * N + i] : 1.0;
        if (wk == 0.0) continue;                  // rule 2: a set without weight is skipped, whatever its solve gave
        const double e = sse[(int64_t)k * N + i];
        ws = fold_term(ws, wk, e);
        bool b = !is_finite(e);
        for (int r = 0; r < P; r++) b |= !is_finite(rows[((int64_t)k * P + r) * N + i]);
        nb += b ? 1 : 0;
    }
    a.wsse[i] = ws;
    a.bad[i] = nb;
}

// rule 3 and the parameter mask, one lane per subject, in place
__global__ __launch_bounds__(kScoreThreads) void scores_finish_kernel(ScoresArgs a, const double* __restrict__ mask,
                                                                       int32_t* __restrict__ n_failed) {
    const int64_t i = (int64_t)blockIdx.x * kScoreThreads + threadIdx.x;
    if (i >= a.N) return;
    const int64_t N = a.N;
    bool f = a.bad[i] > 0 || !is_finite(a.wsse[i]);
    for (int q = 0; q < a.P; q++) f |= !is_finite(a.s[(int64_t)q * N + i]);     // (a weighted sum that overflowed)
    const double nan = __builtin_nan("");
    for (int q = 0; q < a.P; q++) {
        const double m = mask != nullptr ? mask[q] : 1.0;
        const double v = a.s[(int64_t)q * N + i];
        a.s[(int64_t)q * N + i] = m == 0.0 ? 0.0 : (f ? nan : v * m);
    }
    if (f) {
        a.wsse[i] = nan;
        atomicAdd(n_failed, 1);
    }
    a.fail[i] = f ? 1 : 0;
}

// [P][N] -> the caller's [N][P], through a 32 x 32 tile (33-wide rows: no bank conflict on the transposed read)
__global__ __launch_bounds__(256) void scores_transpose_kernel(int64_t N, int P, const double* __restrict__ src,
                                                               double* __restrict__ dst) {
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;       // 32 x 8
    const int64_t i0 = (int64_t)blockIdx.x * 32;
    const int q0 = blockIdx.y * 32;
    for (int r = ty; r < 32; r += 8)
        if (q0 + r < P && i0 + tx < N) tile[r][tx] = src[(int64_t)(q0 + r) * N + i0 + tx];
    __syncthreads();
    for (int r = ty; r < 32; r += 8)
        if (i0 + r < N && q0 + tx < P) dst[(i0 + r) * P + q0 + tx] = tile[tx][r];
}

// the t-th tile of the upper triangle of an nt x nt tile grid, row by row
__device__ __forceinline__ void upper_tile(int t, int nt, int* tq, int* tr) {
    int q = 0;
    while (t >= nt - q) { t -= nt - q; q++; }
    *tq = q;
    *tr = q + t;
}

// grid: x over the subject blocks, y over the upper triangle's tiles; partial[(block * tiles + tile) * 256 + entry]
__global__ __launch_bounds__(kScoreThreads) void scores_cross_partial_kernel(ScoresArgs a, int nt,
                                                                              double* __restrict__ partial) {
    __shared__ double s_q[kCrossTile * kCrossPitch], s_r[kCrossTile * kCrossPitch];
    const int64_t N = a.N;
    const int P = a.P;
    int tq, tr;
    upper_tile(blockIdx.y, nt, &tq, &tr);
    const int lq = threadIdx.x / kCrossTile, lr = threadIdx.x % kCrossTile;
    const int64_t b0 = (int64_t)blockIdx.x * kCrossSubjects;
    const int64_t b1 = b0 + kCrossSubjects < N ? b0 + kCrossSubjects : N;
    double acc = 0.0;
    for (int64_t i0 = b0; i0 < b1; i0 += kCrossSub) {
        __syncthreads();
        // row P is the row of ones; a failed subject's column and whatever lies past the table are zero
        for (int e = threadIdx.x; e < kCrossTile * kCrossSub; e += kScoreThreads) {
            const int row = e / kCrossSub, col = e % kCrossSub;
            const int64_t i = i0 + col;
            const bool live = i < b1 && a.fail[i] == 0;
            const int q = tq * kCrossTile + row, r = tr * kCrossTile + row;
            s_q[row * kCrossPitch + col] = !live || q > P ? 0.0 : (q == P ? 1.0 : a.s[(int64_t)q * N + i]);
            s_r[row * kCrossPitch + col] = !live || r > P ? 0.0 : (r == P ? 1.0 : a.s[(int64_t)r * N + i]);
        }
        __syncthreads();
        const int n = (int)(b1 - i0 < kCrossSub ? b1 - i0 : kCrossSub);
        for (int col = 0; col < n; col++) acc = fma(s_q[lq * kCrossPitch + col], s_r[lr * kCrossPitch + col], acc);
    }
    partial[((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * kScoreThreads + threadIdx.x] = acc;
}

// grid: x over the upper triangle's tiles; the blocks' partial sums in block order, every value to both triangles
__global__ __launch_bounds__(kScoreThreads) void scores_cross_finish_kernel(int P, int nt, int64_t nblk, int ntiles,
                                                                             const double* __restrict__ partial,
                                                                             double* __restrict__ sum,
                                                                             double* __restrict__ cross) {
    int tq, tr;
    upper_tile(blockIdx.x, nt, &tq, &tr);
    const int q = tq * kCrossTile + threadIdx.x / kCrossTile, r = tr * kCrossTile + threadIdx.x % kCrossTile;
    if (q > r || r > P || q >= P) return;
    double v = 0.0;
    for (int64_t b = 0; b < nblk; b++) v += partial[(b * ntiles + blockIdx.x) * kScoreThreads + threadIdx.x];
    if (r == P) {
        if (sum != nullptr) sum[q] = v;
    } else if (cross != nullptr) {
        cross[(int64_t)q * P + r] = v;
        cross[(int64_t)r * P + q] = v;
    }
}
}  // namespace

hipError_t launch_scores_fold(const ScoresArgs& a, int kn, bool first, const double* rows, const double* sse, const double* w,
                              hipStream_t s) {
    const dim3 grid((unsigned)((a.N + kScoreThreads - 1) / kScoreThreads), (unsigned)(a.P + 1));
    hipLaunchKernelGGL(scores_fold_kernel, grid, dim3(kScoreThreads), 0, s, a, kn, first ? 1 : 0, rows, sse, w);
    return hipGetLastError();
}

hipError_t launch_scores_finish(const ScoresArgs& a, const double* mask, int32_t* n_failed, double* score_out_dev, hipStream_t s) {
    hipLaunchKernelGGL(scores_finish_kernel, dim3((unsigned)((a.N + kScoreThreads - 1) / kScoreThreads)), dim3(kScoreThreads), 0,
                       s, a, mask, n_failed);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || score_out_dev == nullptr) return e;
    const dim3 grid((unsigned)((a.N + 31) / 32), (unsigned)((a.P + 31) / 32));
    hipLaunchKernelGGL(scores_transpose_kernel, grid, dim3(256), 0, s, a.N, a.P, a.s, score_out_dev);
    return hipGetLastError();
}

int64_t scores_cross_blocks(int64_t N) { return (N + kCrossSubjects - 1) / kCrossSubjects; }
int scores_cross_tiles(int P) {
    const int nt = (P + 1 + kCrossTile - 1) / kCrossTile;
    return nt * (nt + 1) / 2;
}
size_t scores_cross_partials(int64_t N, int P) { return (size_t)scores_cross_blocks(N) * scores_cross_tiles(P) * kScoreThreads; }

hipError_t launch_scores_cross(const ScoresArgs& a, double* partial, double* sum, double* cross, hipStream_t s) {
    const int nt = (a.P + 1 + kCrossTile - 1) / kCrossTile;
    const int ntiles = scores_cross_tiles(a.P);
    const int64_t nblk = scores_cross_blocks(a.N);
    hipLaunchKernelGGL(scores_cross_partial_kernel, dim3((unsigned)nblk, (unsigned)ntiles), dim3(kScoreThreads), 0, s, a, nt, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(scores_cross_finish_kernel, dim3((unsigned)ntiles), dim3(kScoreThreads), 0, s, a.P, nt, nblk, ntiles, partial,
                       sum, cross);
    return hipGetLastError();
}

}  // namespace cude
