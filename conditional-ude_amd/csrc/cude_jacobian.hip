// Output Jacobians with respect to the shared (network) parameters and the expected-information matrices built from them
// (cude_network_information; the numbered rules in include/cude.h).  The gradient launches compiled with ROWS run with a
// unit adjoint seed (CpepArgs::unit_seed): set k of a launch is live output l0 + k, its lanes' rows [set][P][N] are
// J_io = d yhat_io / d theta and its g_cond [set][N] is jc_io = d yhat_io / d cond_i.  The kernels here fold that table:
//
//   fold      b_i = sum_o w_o jc_io J_io and d_i = sum_o w_o jc_io^2, one lane per (parameter, subject), the outputs of a
//             subject strictly in output order into state that lives in device memory between the launches of a call, every
//             product and every sum rounded on its own (contraction off): no output depends on the chunking.
//   finish    status (FAILED, FLAT), NaN rows of failed subjects, t_i = b_i / sqrt(d_i + pw) for the Schur term.
//   cross     A = sum_i sum_o w_o J_io^T J_io with plain FMAs (the fp64 matrix rate equals the vector rate on this part, and
//             the table is streamed, not re-used).  One workgroup per (block of kCrossSubjects subjects, 16 x 16 tile of the
//             upper triangle); its partial sum lives in device memory between the launches and takes the outputs in order,
//             inside an output the block's subjects in index order, so the association order is fixed by (N, n_out) alone.
//             The finishing kernel adds the blocks in block order and writes every value to both triangles.  The Schur
//             term sum_i t_i t_i^T is the same kernel on the table t with one "output" of weight 1.
//   qform     z C z^T per (subject, output), z staged in LDS, C read through the scalar cache.
#include <hip/hip_runtime.h>

#include "cude_kernels.h"

namespace cude {

namespace {
constexpr int kInfoThreads = 256;
constexpr int kCrossTile = 16;                    // entries of a tile: kCrossTile x kCrossTile, one lane each
constexpr int kCrossSub = 128;                    // subjects staged in LDS at a time (2 x 16 rows: 33 KB) ...
constexpr int kCrossSubjects = 1024;              // ... and per workgroup
constexpr int kCrossPitch = kCrossSub + 1;        // LDS row pitch: the 16 rows a wave reads at once fall into 16 banks
constexpr int kQformLanes = 64;
constexpr double kDblMax = 1.79769313486231570815e308;

__device__ __forceinline__ bool is_finite(double v) { return fabs(v) <= kDblMax; }
__device__ __forceinline__ double masked(const double* __restrict__ mask, int q, double v) {
    if (mask == nullptr) return v;
    const double m = mask[q];
    return m == 0.0 ? 0.0 : v * m;
}
// s + (w * x) * y, every operation rounded on its own
__device__ __forceinline__ double fold_term(double s, double w, double x, double y) {
#pragma clang fp contract(off)
    const double wx = w * x;
    const double p = wx * y;
    return s + p;
}

// grid: x over the subjects, y over the parameters 0 ... P - 1 and, as row P, d_i, the failure count and the jc table
__global__ __launch_bounds__(kInfoThreads) void info_fold_kernel(InfoArgs a, int kn, int l0, int first,
                                                                  const double* __restrict__ rows,
                                                                  const double* __restrict__ jc,
                                                                  const double* __restrict__ sse) {
    const int64_t i = (int64_t)blockIdx.x * kInfoThreads + threadIdx.x;
    if (i >= a.N) return;
    const int64_t N = a.N;
    const int P = a.P;
    const int q = blockIdx.y;
    if (q < P) {
        double s = first ? 0.0 : a.b[(int64_t)q * N + i];
        for (int k = 0; k < kn; k++)
            s = fold_term(s, a.weight(l0 + k), jc[(int64_t)k * N + i], masked(a.mask, q, rows[((int64_t)k * P + q) * N + i]));
        a.b[(int64_t)q * N + i] = s;
        return;
    }
    double d = first ? 0.0 : a.d[i];
    int32_t nb = first ? 0 : a.bad[i];
    for (int k = 0; k < kn; k++) {
        const double g = jc[(int64_t)k * N + i];
        d = fold_term(d, a.weight(l0 + k), g, g);
        bool b = !is_finite(g) || !is_finite(sse[(int64_t)k * N + i]);
        for (int r = 0; r < P; r++) b |= !is_finite(rows[((int64_t)k * P + r) * N + i]);
        nb += b ? 1 : 0;
        a.jc[i * a.n_out + a.out_index(l0 + k)] = g;
    }
    a.d[i] = d;
    a.bad[i] = nb;
}

// one lane per subject: status, the failed subjects' NaNs, the Schur term's table
__global__ __launch_bounds__(kInfoThreads) void info_finish_kernel(InfoArgs a, int32_t* __restrict__ n_failed) {
    const int64_t i = (int64_t)blockIdx.x * kInfoThreads + threadIdx.x;
    if (i >= a.N) return;
    const int64_t N = a.N;
    bool f = a.bad[i] > 0 || !is_finite(a.d[i]);
    for (int q = 0; q < a.P; q++) f |= !is_finite(a.b[(int64_t)q * N + i]);
    const double den = a.d[i] + a.pw;
    const bool flat = !f && !(den > 0.0);
    const double nan = __builtin_nan("");
    const double rs = (f || flat) ? 0.0 : sqrt(den);
    for (int q = 0; q < a.P; q++) {
        const bool off = a.mask != nullptr && a.mask[q] == 0.0;
        const double v = a.b[(int64_t)q * N + i];
        if (f) a.b[(int64_t)q * N + i] = off ? 0.0 : nan;
        a.t[(int64_t)q * N + i] = (f || flat || off) ? 0.0 : v / rs;
    }
    if (f) {
        a.d[i] = nan;
        for (int o = 0; o < a.n_out; o++) { a.jc[i * a.n_out + o] = nan; a.qf[i * a.n_out + o] = nan; }
        atomicAdd(n_failed, 1);
    }
    a.status[i] = (f ? 1 : 0) | (flat ? 2 : 0);
}

// src [K][P][N] -> dst[(i * dst_rows + row0 + k) * P + q] with k' = out_index(l0 + k) - out_index(l0), through a 32 x 32
// tile (33-wide rows: no bank conflict on the transposed read); grid: x over the subjects, y over the parameters, z over K
__global__ __launch_bounds__(256) void info_transpose_kernel(InfoArgs a, int l0, int dst_rows, const double* __restrict__ src,
                                                             int apply_mask, double* __restrict__ dst) {
    __shared__ double tile[32][33];
    const int64_t N = a.N;
    const int P = a.P;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;       // 32 x 8
    const int64_t i0 = (int64_t)blockIdx.x * 32;
    const int q0 = blockIdx.y * 32;
    const int k = blockIdx.z;
    const int row = l0 < 0 ? k : a.out_index(l0 + k) - a.out_index(l0);
    for (int r = ty; r < 32; r += 8)
        if (q0 + r < P && i0 + tx < N) {
            const double v = src[((int64_t)k * P + q0 + r) * N + i0 + tx];
            tile[r][tx] = apply_mask ? masked(a.mask, q0 + r, v) : v;
        }
    __syncthreads();
    for (int r = ty; r < 32; r += 8)
        if (i0 + r < N && q0 + tx < P) dst[((i0 + r) * dst_rows + row) * P + q0 + tx] = tile[tx][r];
}

__global__ __launch_bounds__(kInfoThreads) void info_replicate_kernel(int64_t N, int kn, const double* __restrict__ src,
                                                                       double* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * kInfoThreads + threadIdx.x;
    if (i >= N) return;
    const double v = src[i];
    for (int k = 0; k < kn; k++) dst[(int64_t)k * N + i] = v;
}

// the t-th tile of the upper triangle of an nt x nt tile grid, row by row
__device__ __forceinline__ void upper_tile(int t, int nt, int* tq, int* tr) {
    int q = 0;
    while (t >= nt - q) { t -= nt - q; q++; }
    *tq = q;
    *tr = q + t;
}

// grid: x over the subject blocks, y over the upper triangle's tiles; partial[(block * tiles + tile) * 256 + entry] carries on
// from the launch before (first: from zero).  l0 < 0: one table of weight 1 (the Schur term).
__global__ __launch_bounds__(kInfoThreads) void info_cross_kernel(InfoArgs a, int kn, int l0, int first, int nt,
                                                                   const double* __restrict__ rows,
                                                                   const int32_t* __restrict__ status,
                                                                   double* __restrict__ partial) {
    __shared__ double s_q[kCrossTile * kCrossPitch], s_r[kCrossTile * kCrossPitch];
    const int64_t N = a.N;
    const int P = a.P;
    int tq, tr;
    upper_tile(blockIdx.y, nt, &tq, &tr);
    const int lq = threadIdx.x / kCrossTile, lr = threadIdx.x % kCrossTile;
    const int64_t b0 = (int64_t)blockIdx.x * kCrossSubjects;
    const int64_t b1 = b0 + kCrossSubjects < N ? b0 + kCrossSubjects : N;
    const int64_t slot = ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * kInfoThreads + threadIdx.x;
    double acc = first ? 0.0 : partial[slot];
    for (int k = 0; k < kn; k++) {
        const double w = l0 < 0 ? 1.0 : a.weight(l0 + k);
        const double* tab = rows + (int64_t)k * P * N;
        for (int64_t i0 = b0; i0 < b1; i0 += kCrossSub) {
            __syncthreads();
            // a failed subject's column and whatever lies past the table are zero
            for (int e = threadIdx.x; e < kCrossTile * kCrossSub; e += kInfoThreads) {
                const int row = e / kCrossSub, col = e % kCrossSub;
                const int64_t i = i0 + col;
                const bool live = i < b1 && (status == nullptr || (status[i] & 1) == 0);
                const int q = tq * kCrossTile + row, r = tr * kCrossTile + row;
                s_q[row * kCrossPitch + col] = !live || q >= P ? 0.0 : w * masked(a.mask, q, tab[(int64_t)q * N + i]);
                s_r[row * kCrossPitch + col] = !live || r >= P ? 0.0 : masked(a.mask, r, tab[(int64_t)r * N + i]);
            }
            __syncthreads();
            const int n = (int)(b1 - i0 < kCrossSub ? b1 - i0 : kCrossSub);
            for (int col = 0; col < n; col++) acc = fma(s_q[lq * kCrossPitch + col], s_r[lr * kCrossPitch + col], acc);
        }
    }
    partial[slot] = acc;
}

// grid: x over the upper triangle's tiles; the blocks' partial sums in block order, every value to both triangles
__global__ __launch_bounds__(kInfoThreads) void info_cross_finish_kernel(int P, int nt, int64_t nblk, int ntiles,
                                                                          const double* __restrict__ partial,
                                                                          double* __restrict__ dst) {
    int tq, tr;
    upper_tile(blockIdx.x, nt, &tq, &tr);
    const int q = tq * kCrossTile + threadIdx.x / kCrossTile, r = tr * kCrossTile + threadIdx.x % kCrossTile;
    if (q > r || r >= P) return;
    double v = 0.0;
    for (int64_t b = 0; b < nblk; b++) v += partial[(b * ntiles + blockIdx.x) * kInfoThreads + threadIdx.x];
    dst[(int64_t)q * P + r] = v;
    dst[(int64_t)r * P + q] = v;
}

// S = A - X, entry by entry (both symmetric bit for bit, so S is)
__global__ __launch_bounds__(kInfoThreads) void info_schur_kernel(int n, const double* __restrict__ gn,
                                                                   const double* __restrict__ x, double* __restrict__ schur) {
    const int e = blockIdx.x * kInfoThreads + threadIdx.x;
    if (e < n) schur[e] = gn[e] - x[e];
}

// grid: x over the subjects (one wave each), y over the sets of the launch; dynamic LDS: [P][64] doubles
__global__ __launch_bounds__(kQformLanes) void info_qform_kernel(InfoArgs a, int l0, int profiled,
                                                                  const double* __restrict__ rows,
                                                                  const double* __restrict__ jc,
                                                                  const double* __restrict__ cov) {
    extern __shared__ double s_z[];
    const int lane = threadIdx.x;
    const int64_t gid = (int64_t)blockIdx.x * kQformLanes + lane;
    const bool active = gid < a.N;
    const int64_t i = active ? gid : a.N - 1;
    const int64_t N = a.N;
    const int P = a.P;
    const int k = blockIdx.y;
    const int32_t st = a.status[i];
    const double coef = (profiled && (st & 2) == 0) ? jc[(int64_t)k * N + i] / (a.d[i] + a.pw) : 0.0;
    for (int q = 0; q < P; q++) {
#pragma clang fp contract(off)
        const double p = coef * a.b[(int64_t)q * N + i];
        s_z[q * kQformLanes + lane] = masked(a.mask, q, rows[((int64_t)k * P + q) * N + i]) - p;
    }
    double acc = 0.0;
    for (int q = 0; q < P; q++) {
        double y = 0.0;
        for (int r = 0; r < P; r++) y = fma(cov[(int64_t)q * P + r], s_z[r * kQformLanes + lane], y);
        acc = fma(s_z[q * kQformLanes + lane], y, acc);
    }
    if (active) a.qf[i * a.n_out + a.out_index(l0 + k)] = (st & 1) ? __builtin_nan("") : acc;
}
}  // namespace

hipError_t launch_info_replicate(int64_t N, int kn, const double* src, double* dst, hipStream_t s) {
    hipLaunchKernelGGL(info_replicate_kernel, dim3((unsigned)((N + kInfoThreads - 1) / kInfoThreads)), dim3(kInfoThreads), 0, s, N,
                       kn, src, dst);
    return hipGetLastError();
}

hipError_t launch_info_fold(const InfoArgs& a, int kn, int l0, bool first, const double* rows, const double* jc, const double* sse,
                            hipStream_t s) {
    const dim3 grid((unsigned)((a.N + kInfoThreads - 1) / kInfoThreads), (unsigned)(a.P + 1));
    hipLaunchKernelGGL(info_fold_kernel, grid, dim3(kInfoThreads), 0, s, a, kn, l0, first ? 1 : 0, rows, jc, sse);
    return hipGetLastError();
}

hipError_t launch_info_finish(const InfoArgs& a, int32_t* n_failed, hipStream_t s) {
    hipLaunchKernelGGL(info_finish_kernel, dim3((unsigned)((a.N + kInfoThreads - 1) / kInfoThreads)), dim3(kInfoThreads), 0, s, a,
                       n_failed);
    return hipGetLastError();
}

hipError_t launch_info_transpose(const InfoArgs& a, int kn, int l0, int dst_rows, const double* src, bool apply_mask, double* dst,
                                 hipStream_t s) {
    const dim3 grid((unsigned)((a.N + 31) / 32), (unsigned)((a.P + 31) / 32), (unsigned)kn);
    hipLaunchKernelGGL(info_transpose_kernel, grid, dim3(256), 0, s, a, l0, dst_rows, src, apply_mask ? 1 : 0, dst);
    return hipGetLastError();
}

static int64_t info_cross_blocks(int64_t N) { return (N + kCrossSubjects - 1) / kCrossSubjects; }
static int info_cross_nt(int P) { return (P + kCrossTile - 1) / kCrossTile; }
static int info_cross_tiles(int P) { return info_cross_nt(P) * (info_cross_nt(P) + 1) / 2; }
size_t info_cross_partials(int64_t N, int P) { return (size_t)info_cross_blocks(N) * info_cross_tiles(P) * kInfoThreads; }

hipError_t launch_info_cross(const InfoArgs& a, int kn, int l0, bool first, const double* rows, const int32_t* status,
                             double* partial, hipStream_t s) {
    const dim3 grid((unsigned)info_cross_blocks(a.N), (unsigned)info_cross_tiles(a.P));
    hipLaunchKernelGGL(info_cross_kernel, grid, dim3(kInfoThreads), 0, s, a, kn, l0, first ? 1 : 0, info_cross_nt(a.P), rows,
                       status, partial);
    return hipGetLastError();
}

hipError_t launch_info_cross_finish(const InfoArgs& a, const double* partial, double* dst, hipStream_t s) {
    const int ntiles = info_cross_tiles(a.P);
    hipLaunchKernelGGL(info_cross_finish_kernel, dim3((unsigned)ntiles), dim3(kInfoThreads), 0, s, a.P, info_cross_nt(a.P),
                       info_cross_blocks(a.N), ntiles, partial, dst);
    return hipGetLastError();
}

hipError_t launch_info_schur(int P, const double* gn, const double* x, double* schur, hipStream_t s) {
    const int n = P * P;
    hipLaunchKernelGGL(info_schur_kernel, dim3((unsigned)((n + kInfoThreads - 1) / kInfoThreads)), dim3(kInfoThreads), 0, s, n, gn, x,
                       schur);
    return hipGetLastError();
}

hipError_t launch_info_qform(const InfoArgs& a, int kn, int l0, bool profiled, const double* rows, const double* jc,
                             const double* cov, hipStream_t s) {
    const size_t lds = sizeof(double) * (size_t)a.P * kQformLanes;
    if (lds > 65536) {
        const hipError_t e = hipFuncSetAttribute((const void*)info_qform_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const dim3 grid((unsigned)((a.N + kQformLanes - 1) / kQformLanes), (unsigned)kn);
    hipLaunchKernelGGL(info_qform_kernel, grid, dim3(kQformLanes), lds, s, a, l0, profiled ? 1 : 0, rows, jc, cov);
    return hipGetLastError();
}

}  // namespace cude
