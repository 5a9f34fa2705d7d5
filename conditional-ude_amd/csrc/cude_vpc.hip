// Visual predictive check by subject group (cude_vpc, include/cude.h): the reductions behind the simulation that cude_npde's
// kernels leave as y [K][R][subjects] (launch_npde_observe).
//
// Replaces: nothing in the reference repo -- it plots its diagnostics by subject type (`train_data.types`) but has no
// simulation-based check of the population model.  The host route these kernels stand for is a download of every simulated
// observation and numpy.quantile over subjects for every (simulation, row, group), then over simulations.
//
// The direction is new: the other reductions of the library (cude_predictive.hip, cude_bootstrap.hip, cude_npde.hip) reduce
// over the set dimension for one subject, at most 4096 values per column; here a column is one (simulation, row) over the n
// MEMBERS of a group -- any length up to N -- read through the group's list of subject indices.  Only the 2 L <= 16 order
// statistics of rule 3 are wanted per column.
//
//   * vpc_tile_kernel (n <= 4096): the column is gathered into the shared sorting tile (cude_tilesort.h), [Kp][C] doubles
//     padded with +Inf, C = min(64, 8192 / Kp) neighbouring columns (rows of one simulation, then of the next) per workgroup,
//     and the ranks are read off.
//   * vpc_select_kernel (longer columns; every column with option "vpc_select"): one 256-thread workgroup per column, which
//     never leaves device memory -- at 1e5 subjects it is 0.8 MB and stays in an XCD's 4 MiB L2 over the nine passes.  The
//     double is mapped to a 64-bit key of the same order (sign bit flipped for positive values, all bits for negative ones)
//     and the key of every wanted lo rank is found digit by digit, 8 bits per pass from the top: a pass counts, per rank,
//     the digits of the elements that share the rank's prefix in a 256-bin LDS histogram, a lane per rank walks its
//     histogram to the bin that holds the rank and appends the digit.  The L descents share each pass over the column, and
//     ranks whose prefixes still agree share one histogram (after the sign and exponent digits that is most of them).  The
//     top digits of a column of like-sized values are nearly all equal: a wave whose lanes all hold one digit adds its
//     count with one LDS atomic rather than 64 colliding ones.  After eight passes the prefix IS the key of x_lo, the bin's
//     count the number of elements equal to it; where the next rank is not among those, one more pass takes the smallest
//     key above it (LDS atomicMin) -- x_hi.  Keys map back to the column's own bits: selected, not computed.
//   * vpc_interval_kernel: rule 6, the K quantiles of a (group, row, level) on the sorting tile as the predictive bands',
//     left-out simulations padded with +Inf, ranks from n_sims_used[g].
//   * vpc_bad_obs_kernel, vpc_flag_kernel, vpc_count_kernel, vpc_nan_kernel: rule 2's and rule 5's flags and counts.
#include <hip/hip_runtime.h>

#include "cude_kernels.h"
#include "cude_observe.h"
#include "cude_tilesort.h"

namespace cude {

namespace {
constexpr int kVpcThreads = kTileSortThreads;
constexpr int kVpcBatch = 4;                      // elements a lane of the select kernel fetches before it counts them
constexpr int kVpcTileMax = kPredMaxSets;        // the longest column the sorting tile takes (4096: two columns per tile)

// rule 3's position of level q among n values
__device__ __forceinline__ void vpc_rank(int n, double q, int* lo, int* hi, double* frac) {
#pragma clang fp contract(off)
    const double h = (double)(n - 1) * q;
    const double fl = floor(h);
    const int l = (int)fl;
    *lo = l;
    *hi = l + 1 < n - 1 ? l + 1 : n - 1;
    *frac = h - fl;
}
// rule 3's value, anchored at the nearer neighbour; every operation rounded on its own
__device__ __forceinline__ double vpc_lerp(double x_lo, double x_hi, double g) {
#pragma clang fp contract(off)
    const double d = x_hi - x_lo;
    if (g >= 0.5) {
        const double w = 1.0 - g;
        const double p = d * w;
        return x_hi - p;
    }
    const double p = d * g;
    return x_lo + p;
}

// the 64-bit key whose unsigned order is the doubles' order (-0.0 just below +0.0), and back
__device__ __forceinline__ unsigned long long vpc_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull);
}
__device__ __forceinline__ double vpc_unkey(unsigned long long k) {
    const unsigned long long b = k ^ ((k >> 63) ? 0x8000000000000000ull : ~0ull);
    return __longlong_as_double((long long)b);
}

__global__ __launch_bounds__(kVpcThreads) void vpc_bad_obs_kernel(int64_t N, int R, const double* __restrict__ obs,
                                                                  const double* __restrict__ sigma, uint8_t* __restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * kVpcThreads + threadIdx.x;
    if (i >= N) return;
    bool ok = finite_value(sigma[i]);
    for (int r = 0; r < R; r++) ok = ok && finite_value(obs[(int64_t)(r + 1) * N + i]);
    bad[i] = ok ? 0 : 1;
}

__global__ __launch_bounds__(kVpcThreads) void vpc_flag_kernel(int64_t N, int G, const int32_t* __restrict__ grp,
                                                               const uint8_t* __restrict__ used, uint8_t* __restrict__ sim_bad,
                                                               int32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * kVpcThreads + threadIdx.x;
    if (i >= N) return;
    const int k = blockIdx.y;
    const int g = grp[i];
    if (g < 0 || used[(int64_t)k * N + i]) return;
    sim_bad[(int64_t)k * G + g] = 1;                 // (every writer stores the same byte)
    atomicOr(&status[i], kVpcFailedSims);
}

__global__ void vpc_count_kernel(int K, int G, const uint8_t* __restrict__ sim_bad, int32_t* __restrict__ n_used) {
    const int g = threadIdx.x;
    if (g >= G) return;
    int32_t n = 0;
    for (int k = 0; k < K; k++) n += sim_bad[(int64_t)k * G + g] ? 0 : 1;
    n_used[g] = n;
}

// a group without members: NaN in its entries of out [K][G][R][L]
__global__ __launch_bounds__(kVpcThreads) void vpc_nan_kernel(VpcColumnsArgs a) {
    const int idx = blockIdx.x * kVpcThreads + threadIdx.x;
    const int RL = a.R * a.L;
    if (idx >= a.K * RL) return;
    const int k = idx / RL, e = idx - k * RL;
    a.out[((int64_t)k * a.G + a.g) * RL + e] = __builtin_nan("");
}

__global__ __launch_bounds__(kVpcThreads) void vpc_tile_kernel(VpcColumnsArgs a, int lgC, int Kp) {
    extern __shared__ double s_v[];                  // [Kp][C]
    const int tid = threadIdx.x;
    const int C = 1 << lgC;
    const int n_cols = a.K * a.R;
    const int q0 = blockIdx.x * C;                   // first column of the tile: column q = k R + r
    const double inf = __builtin_huge_val();
    tile_fill(s_v, C, lgC, Kp, tid, [&](int e, int cc) {
        const int q = q0 + cc;
        return (e < a.n && q < n_cols) ? a.y[(int64_t)q * a.N + a.members[e]] : inf;
    });
    tile_sort_ascending(s_v, lgC, Kp, tid);          // (cude_tilesort.h; its first step is a barrier)
    for (int idx = tid; idx < a.L << lgC; idx += kVpcThreads) {
        const int l = idx % a.L, cc = idx / a.L;
        const int q = q0 + cc;
        if (q >= n_cols) continue;
        const int k = q / a.R, r = q - k * a.R;
        int lo, hi;
        double frac;
        vpc_rank(a.n, a.levels[l], &lo, &hi, &frac);
        const double v = vpc_lerp(s_v[(lo << lgC) + cc], s_v[(hi << lgC) + cc], frac);
        const bool bad = a.sim_bad != nullptr && a.sim_bad[(int64_t)k * a.G + a.g] != 0;
        a.out[(((int64_t)k * a.G + a.g) * a.R + r) * a.L + l] = bad ? __builtin_nan("") : v;
    }
}

// one count into a histogram bin; a wave whose active lanes all hold the same digit adds once
__device__ __forceinline__ void vpc_hist_add(uint32_t* hist, unsigned digit) {
    const unsigned long long active = __ballot(1);
    const unsigned d0 = (unsigned)__builtin_amdgcn_readfirstlane((int)digit);
    if (__ballot(digit == d0) == active) {
        if ((int)__lane_id() == __ffsll((long long)active) - 1) atomicAdd(&hist[d0], (uint32_t)__popcll(active));
    } else {
        atomicAdd(&hist[digit], 1u);
    }
}

__global__ __launch_bounds__(kVpcThreads) void vpc_select_kernel(VpcColumnsArgs a) {
    __shared__ uint32_t s_hist[kVpcMaxLevels][256];
    __shared__ unsigned long long s_prefix[kVpcMaxLevels], s_min[kVpcMaxLevels];
    __shared__ double s_frac[kVpcMaxLevels];
    __shared__ int32_t s_rem[kVpcMaxLevels], s_eq[kVpcMaxLevels], s_own[kVpcMaxLevels], s_tie[kVpcMaxLevels];
    const int tid = threadIdx.x;
    const int L = a.L, n = a.n;
    const int q = blockIdx.x;                        // column q = k R + r
    const int k = q / a.R, r = q - k * a.R;
    double* const out = a.out + (((int64_t)k * a.G + a.g) * a.R + r) * L;
    if (a.sim_bad != nullptr && a.sim_bad[(int64_t)k * a.G + a.g] != 0) {       // (the whole workgroup)
        if (tid < L) out[tid] = __builtin_nan("");
        return;
    }
    const double* __restrict__ const col = a.y + (int64_t)q * a.N;
    const int32_t* __restrict__ const members = a.members;
    if (tid < L) {
        int lo, hi;
        double frac;
        vpc_rank(n, a.levels[tid], &lo, &hi, &frac);
        s_rem[tid] = lo;                             // the rank among the elements that share the prefix
        s_tie[tid] = hi == lo ? 1 : 0;               // x_hi = x_lo
        s_frac[tid] = frac;
        s_prefix[tid] = 0ull;
        s_own[tid] = 0;                              // the first rank with the same prefix: its histogram is shared
        s_min[tid] = ~0ull;
    }
    __syncthreads();
    for (int pass = 0; pass < 8; pass++) {
        const int shift = 56 - 8 * pass;
        for (int idx = tid; idx < L * 256; idx += kVpcThreads) (&s_hist[0][0])[idx] = 0u;
        unsigned long long prefix[kVpcMaxLevels];
        bool own[kVpcMaxLevels];
#pragma unroll
        for (int l = 0; l < kVpcMaxLevels; l++) {
            prefix[l] = l < L ? s_prefix[l] : 0ull;
            own[l] = l < L && s_own[l] == l;
        }
        __syncthreads();
        // (the wave votes of vpc_hist_add keep the compiler from unrolling: four elements' gathers are requested by hand
        // before the first is counted)
        for (int j0 = tid; j0 < n; j0 += kVpcBatch * kVpcThreads) {
            unsigned long long keys[kVpcBatch];
#pragma unroll
            for (int u = 0; u < kVpcBatch; u++) {
                const int j = j0 + u * kVpcThreads;
                keys[u] = j < n ? vpc_key(col[members[j]]) : 0ull;
            }
#pragma unroll
            for (int u = 0; u < kVpcBatch; u++) {
                if (j0 + u * kVpcThreads < n) {
                    const unsigned long long top = pass ? keys[u] >> (shift + 8) : 0ull;
                    const unsigned digit = (unsigned)(keys[u] >> shift) & 255u;
#pragma unroll
                    for (int l = 0; l < kVpcMaxLevels; l++)
                        if (own[l] && top == prefix[l]) vpc_hist_add(s_hist[l], digit);
                }
            }
        }
        __syncthreads();
        if (tid < L) {
            const uint32_t* const h = s_hist[s_own[tid]];
            const uint32_t rem = (uint32_t)s_rem[tid];
            uint32_t cum = 0, c = 0;
            int d = 0;
            for (; d < 255; d++) {
                c = h[d];
                if (rem < cum + c) break;
                cum += c;
            }
            if (d == 255) c = h[255];
            s_rem[tid] = (int32_t)(rem - cum);
            s_eq[tid] = (int32_t)c;
            s_prefix[tid] = (s_prefix[tid] << 8) | (unsigned long long)d;
        }
        __syncthreads();
        if (tid < L) {
            int o = tid;
            for (int l = tid - 1; l >= 0; l--)
                if (s_prefix[l] == s_prefix[tid]) o = l;
            s_own[tid] = o;
        }
        __syncthreads();
    }
    // s_prefix: the key of x_lo; s_eq elements equal it and x_lo is number s_rem among them
    bool need = false, tie[kVpcMaxLevels];
#pragma unroll
    for (int l = 0; l < kVpcMaxLevels; l++) {
        tie[l] = l >= L || s_tie[l] != 0 || s_rem[l] + 1 < s_eq[l];      // (... the next rank is one of the equals)
        need = need || !tie[l];
    }
    if (need) {                                      // (the whole workgroup: every thread read the same LDS words)
        unsigned long long key_lo[kVpcMaxLevels], best[kVpcMaxLevels];
#pragma unroll
        for (int l = 0; l < kVpcMaxLevels; l++) {
            key_lo[l] = tie[l] ? ~0ull : s_prefix[l];                    // (nothing lies above ~0: no candidate)
            best[l] = ~0ull;
        }
#pragma unroll 4
        for (int j = tid; j < n; j += kVpcThreads) {
            const unsigned long long key = vpc_key(col[members[j]]);
#pragma unroll
            for (int l = 0; l < kVpcMaxLevels; l++)
                if (key > key_lo[l] && key < best[l]) best[l] = key;
        }
#pragma unroll
        for (int l = 0; l < kVpcMaxLevels; l++)
            if (l < L && best[l] != ~0ull) atomicMin(&s_min[l], best[l]);
        __syncthreads();
    }
    if (tid < L) {
        const double x_lo = vpc_unkey(s_prefix[tid]);
        const bool same = s_tie[tid] != 0 || s_rem[tid] + 1 < s_eq[tid];
        const double x_hi = same ? x_lo : vpc_unkey(s_min[tid]);
        out[tid] = vpc_lerp(x_lo, x_hi, s_frac[tid]);
    }
}

__global__ __launch_bounds__(kVpcThreads) void vpc_interval_kernel(VpcIntervalArgs a, int lgC, int Kp) {
    extern __shared__ double s_v[];                  // [Kp][TC]
    const int tid = threadIdx.x;
    const int TC = 1 << lgC;
    const int RL = a.R * a.L, n_cols = a.G * RL;     // column q = (g R + r) L + l
    const int q0 = blockIdx.x * TC;
    const double inf = __builtin_huge_val();
    tile_fill(s_v, TC, lgC, Kp, tid, [&](int k, int cc) {
        const int q = q0 + cc;
        double v = inf;
        if (k < a.K && q < n_cols && a.sim_bad[(int64_t)k * a.G + q / RL] == 0) v = a.sim_q[(int64_t)k * n_cols + q];
        return v;
    });
    tile_sort_ascending(s_v, lgC, Kp, tid);
    for (int idx = tid; idx < a.C << lgC; idx += kVpcThreads) {
        const int c = idx % a.C, cc = idx / a.C;
        const int q = q0 + cc;
        if (q >= n_cols) continue;
        const int g = q / RL;
        const int n = a.n_used[g];
        double v = __builtin_nan("");
        if (n > 0 && a.n_members[g] > 0) {
            int lo, hi;
            double frac;
            vpc_rank(n, a.ci_levels[c], &lo, &hi, &frac);
            v = vpc_lerp(s_v[(lo << lgC) + cc], s_v[(hi << lgC) + cc], frac);
        }
        a.ci[(int64_t)q * a.C + c] = v;
    }
}
}  // namespace

hipError_t launch_vpc_bad_obs(int64_t N, int R, const double* obs, const double* sigma, uint8_t* bad, hipStream_t s) {
    if (N < 1 || R < 1 || !obs || !sigma || !bad) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vpc_bad_obs_kernel, dim3((unsigned)((N + kVpcThreads - 1) / kVpcThreads)), dim3(kVpcThreads), 0, s, N, R, obs,
                       sigma, bad);
    return hipGetLastError();
}

hipError_t launch_vpc_flag(int64_t N, int K, int G, const int32_t* grp, const uint8_t* used, uint8_t* sim_bad, int32_t* status,
                           hipStream_t s) {
    if (N < 1 || K < 1 || K > kPredMaxSets || G < 1 || G > kVpcMaxGroups || !grp || !used || !sim_bad || !status)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(vpc_flag_kernel, dim3((unsigned)((N + kVpcThreads - 1) / kVpcThreads), (unsigned)K), dim3(kVpcThreads), 0, s, N,
                       G, grp, used, sim_bad, status);
    return hipGetLastError();
}

hipError_t launch_vpc_columns(const VpcColumnsArgs& a, bool force_select, hipStream_t s) {
    if (a.K < 1 || a.K > kPredMaxSets || a.R < 1 || a.R > kNpdeMaxRows || a.G < 1 || a.G > kVpcMaxGroups || a.g < 0 || a.g >= a.G ||
        a.L < 1 || a.L > kVpcMaxLevels || a.n < 0 || a.n > a.N || !a.y || !a.levels || !a.out || (a.n > 0 && !a.members))
        return hipErrorInvalidValue;
    const int n_cols = a.K * a.R;
    if (a.n == 0) {
        hipLaunchKernelGGL(vpc_nan_kernel, dim3((unsigned)((n_cols * a.L + kVpcThreads - 1) / kVpcThreads)), dim3(kVpcThreads), 0, s, a);
    } else if (a.n > kVpcTileMax || force_select) {
        hipLaunchKernelGGL(vpc_select_kernel, dim3((unsigned)n_cols), dim3(kVpcThreads), 0, s, a);
    } else {
        return tile_launch(vpc_tile_kernel, tile_geometry(a.n), n_cols, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_vpc_count(int K, int G, const uint8_t* sim_bad, int32_t* n_used, hipStream_t s) {
    if (K < 1 || G < 1 || G > kVpcMaxGroups || !sim_bad || !n_used) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vpc_count_kernel, dim3(1), dim3(64), 0, s, K, G, sim_bad, n_used);
    return hipGetLastError();
}

hipError_t launch_vpc_interval(const VpcIntervalArgs& a, hipStream_t s) {
    if (a.K < 1 || a.K > kPredMaxSets || a.G < 1 || a.G > kVpcMaxGroups || a.R < 1 || a.R > kNpdeMaxRows || a.L < 1 ||
        a.L > kVpcMaxLevels || a.C < 1 || a.C > kVpcMaxLevels || !a.sim_q || !a.sim_bad || !a.n_used || !a.n_members ||
        !a.ci_levels || !a.ci)
        return hipErrorInvalidValue;
    return tile_launch(vpc_interval_kernel, tile_geometry(a.K), a.G * a.R * a.L, s, a);
}

}  // namespace cude
