// The LDS tile of columns and the bitonic sorting network over it: the ONE statement of the frame of the four kernels that
// read exact order statistics off a set dimension -- predictive_select_kernel (cude_predictive.hip: sample trajectories per
// (subject, time)), bootstrap_reduce_kernel (cude_bootstrap.hip: replicate estimates per subject), vpc_tile_kernel and
// vpc_interval_kernel (cude_vpc.hip: a group's members per (simulation, row); simulations per (group, row, level)).  Here:
// the tile's geometry and launch (host), its fill and its sort (device).  What a kernel does between and after them -- the
// in-order walks, the read-offs -- is its own.
//
// Tile: [Kp][C] doubles, Kp a power of two, C = 1 << lgC columns, element e of column c at e * C + c, padded with +Inf
// behind a column's own values.  All kTileSortThreads threads of the workgroup call the device functions; every
// compare-exchange stays inside its column and sorting is a permutation: afterwards element e of a column is its e-th
// smallest value, one of its own.
//
// CUDE_TILE_GEOMETRY_ONLY: the constants and tile_geometry alone, for a host test that includes this file
// (tests/cpp/replicate_passes.cpp).
#pragma once
#ifndef CUDE_TILE_GEOMETRY_ONLY
#include <hip/hip_runtime.h>
#endif
#include <cstddef>
#include <cstdint>

namespace cude {

constexpr int kTileSortThreads = 256;
constexpr int kTileSortDoubles = 8192;     // 64 KiB: the largest tile
constexpr int kTileSortMaxCols = 64;
constexpr int kTileSortPairs = kTileSortDoubles / 2 / kTileSortThreads;     // compare-exchanges per thread and pass

// The tile of columns of K values: Kp = K rounded up to a power of two, C = min(64, 8192 / Kp) = 1 << lgC columns, its LDS
// (at most 64 KiB per workgroup)
struct TileGeometry {
    int lgC, Kp, C;
    size_t lds;
};
inline TileGeometry tile_geometry(int K) {
    int Kp = 1, lgC = 0;
    while (Kp < K) Kp <<= 1;
    const int C = kTileSortDoubles / Kp < kTileSortMaxCols ? kTileSortDoubles / Kp : kTileSortMaxCols;
    while ((1 << lgC) < C) lgC++;
    return {lgC, Kp, C, sizeof(double) * (size_t)Kp * C};
}

#ifndef CUDE_TILE_GEOMETRY_ONLY
// One workgroup per tile of g.C of the n_cols columns; the kernel's last two parameters are (lgC, Kp).
template <class... Params, class... Args>
hipError_t tile_launch(void (*kernel)(Params...), const TileGeometry& g, int64_t n_cols, hipStream_t s, const Args&... args) {
    // (the largest tile and a kernel's static bytes together pass the 64 KiB a launch may use unasked)
    const hipError_t attr = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                (int)(sizeof(double) * kTileSortDoubles));
    if (attr != hipSuccess) return attr;
    const int64_t tiles = (n_cols + g.C - 1) / g.C;
    hipLaunchKernelGGL(kernel, dim3((unsigned)tiles), dim3(kTileSortThreads), g.lds, s, args..., g.lgC, g.Kp);
    return hipGetLastError();
}

// The fill: element e of column cc of the tile is value(e, cc) -- the kernel's own gather, which answers +Inf for an element
// behind the column's own values and for a column behind the last.  No barrier: the caller's next step brings one.
template <class Value>
__device__ __forceinline__ void tile_fill(double* s_v, int C, int lgC, int Kp, int tid, Value value) {
    const int n_el = Kp << lgC;
    for (int idx = tid; idx < n_el; idx += kTileSortThreads) {
        const int cc = idx & (C - 1), e = idx >> lgC;
        s_v[idx] = value(e, cc);
    }
}

// ascending; pair p of column cc compares elements lo < hi = lo + j.  Ends with a barrier: every thread may read the tile.
__device__ __forceinline__ void tile_sort_ascending(double* s_v, int lgC, int Kp, int tid) {
    const int C = 1 << lgC;
    const int n_pair = (Kp << lgC) >> 1;
    for (int k = 2; k <= Kp; k <<= 1) {
        for (int j = k >> 1; j >= 1; j >>= 1) {
            __syncthreads();
            // a pass's pairs are disjoint: all of a thread's reads are requested before its first exchange is written, so
            // the pass waits for one LDS round trip, not for one per pair
            int ia[kTileSortPairs], ib[kTileSortPairs];
            double x[kTileSortPairs], y[kTileSortPairs];
#pragma unroll
            for (int u = 0; u < kTileSortPairs; u++) {
                const int idx = tid + u * kTileSortThreads;
                const int cc = idx & (C - 1), p = idx >> lgC;
                const int lo = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                const bool up = (lo & k) == 0;
                ia[u] = (lo << lgC) + cc;
                ib[u] = ((lo | j) << lgC) + cc;
                if (idx < n_pair) {
                    x[u] = s_v[up ? ia[u] : ib[u]];      // ascending runs keep (x, y) in place order, descending ones swapped:
                    y[u] = s_v[up ? ib[u] : ia[u]];      // one test x > y for both
                    if (!up) { const int t = ia[u]; ia[u] = ib[u]; ib[u] = t; }
                }
            }
#pragma unroll
            for (int u = 0; u < kTileSortPairs; u++) {
                if (tid + u * kTileSortThreads < n_pair && x[u] > y[u]) { s_v[ia[u]] = y[u]; s_v[ib[u]] = x[u]; }
            }
        }
    }
    __syncthreads();
}

#endif  // CUDE_TILE_GEOMETRY_ONLY

}  // namespace cude
