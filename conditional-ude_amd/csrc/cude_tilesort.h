// The bitonic sorting network over an LDS tile of columns: the ONE statement of the exact order statistics the reductions
// over a set dimension read off (cude_predictive.hip: sample trajectories per (subject, time); cude_bootstrap.hip: replicate
// estimates per subject).
//
// Tile: [Kp][C] doubles, Kp a power of two, C = 1 << lgC columns, element e of column c at e * C + c, padded with +Inf
// behind a column's own values.  All kTileSortThreads threads of the workgroup call it; every compare-exchange stays inside
// its column and sorting is a permutation: afterwards element e of a column is its e-th smallest value, one of its own.
#pragma once
#include <hip/hip_runtime.h>

namespace cude {

constexpr int kTileSortThreads = 256;
constexpr int kTileSortDoubles = 8192;     // 64 KiB: the largest tile
constexpr int kTileSortMaxCols = 64;
constexpr int kTileSortPairs = kTileSortDoubles / 2 / kTileSortThreads;     // compare-exchanges per thread and pass

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

// LDS of a tile of K values per column and its columns: C = min(64, 8192 / Kp), at most 64 KiB per workgroup
inline size_t tile_sort_lds_bytes(int K, int* tile_cols) {
    int Kp = 1;
    while (Kp < K) Kp <<= 1;
    const int C = kTileSortDoubles / Kp < kTileSortMaxCols ? kTileSortDoubles / Kp : kTileSortMaxCols;
    if (tile_cols) *tile_cols = C;
    return sizeof(double) * (size_t)Kp * C;
}

}  // namespace cude
