// Prediction discrepancies and npde (cude_npde, include/cude.h): the kernels around the multi-set dense-output launch.
//
// Replaces: nothing in the reference repo -- it has no simulation-based diagnostic of the population model.  The host loop
// these kernels stand for is n_sims x (cude_set_params, cude_simulate, a download of the trajectories) and numpy's moments,
// Cholesky factor and counts per subject (Brendel et al. 2006; Comets et al. 2008).
//
//   * npde_place_kernel: rule 2's conditional sets  prior_mean + prior_sd z  (or the z alone for cude_npde_draws); one thread
//     per (subject, set), neighbouring threads = neighbouring subjects.
//   * npde_observe_kernel: rule 4.  The solve's slab is [K][subjects][T][NS] -- the R values of one (set, subject) are NS
//     doubles apart, neighbouring subjects T * NS apart -- so the simulated observations are written to a table of their own,
//     y [K][R][subjects], where everything the reduction reads is contiguous over subjects; the caller's noise is uploaded
//     into that table and turned into observations in place.  used [K][subjects]: every row finite (rule 5).
//   * npde_reduce_kernel: rules 5 ... 9.  A workgroup takes a tile of C neighbouring subjects; per subject the mean m [R], the
//     packed lower triangle of C, then L [R (R + 1) / 2], y_obs then w_obs [R] and the decorrelated counts stay in LDS,
//     entry-major with the subject fastest (neighbouring lanes = neighbouring subjects: 8-byte accesses without bank
//     conflicts); C = min(64, 64 KiB / bytes per subject) -- 64 up to R = 10, 14 at R = 31.  Every floating-point sum of the
//     rules is defined per entry, sequentially in k, so the lanes are spread over (row, subject) for the means and the pd
//     counts, over (triangle entry, subject) for C, one lane per subject for the factorisation, and over (simulation group,
//     subject) for the forward substitution, whose counts are integers and meet in LDS atomics.  The substitution keeps a
//     simulation's w and the lane's counts in registers, unrolled for 8, 16 or 31 rows (three instances of the kernel).
#include <algorithm>

#include "cude_kernels.h"
#include "cude_observe.h"
#include "cude_rng.h"

namespace cude {

namespace {
constexpr int kNpdeThreads = 256;
constexpr int kNpdeTileBytes = 65536;
constexpr int kNpdeMaxCols = 64;
constexpr double kNpdePivotTol = 9.094947017729282379150390625e-13;       // 2^-40

// rule 2: prior_mean + prior_sd z, the product rounded, then the sum
__device__ __forceinline__ double npde_effect(double mean, double sd, double z) {
#pragma clang fp contract(off)
    const double d = sd * z;
    return mean + d;
}
// rule 6: acc + (a - ma) (b - mb)
__device__ __forceinline__ double npde_cross_add(double acc, double a, double ma, double b, double mb) {
#pragma clang fp contract(off)
    const double da = a - ma, db = b - mb;
    const double q = da * db;
    return acc + q;
}
// rule 8: acc - a b
__device__ __forceinline__ double npde_mul_sub(double acc, double a, double b) {
#pragma clang fp contract(off)
    const double q = a * b;
    return acc - q;
}

// Wichura (1988), Algorithm AS241, PPND16: the normal quantile of p in (0, 1), relative accuracy about 1e-16
__device__ double npde_ppnd16(double p) {
    const double q = p - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
                                4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                             1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
        const double den = ((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
                               2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
                            4.2313330701600911252e+1) * r + 1.0;
        return num / den;
    }
    double r = q < 0.0 ? p : 1.0 - p;
    r = sqrt(-log(r));
    double x;
    if (r <= 5.0) {
        r = r - 1.6;
        const double num = ((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
                               1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
                            4.63033784615654529590e+0) * r + 1.42343711074968357734e+0;
        const double den = ((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
                               1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
                            2.05319162663775882187e+0) * r + 1.0;
        x = num / den;
    } else {
        r = r - 5.0;
        const double num = ((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
                               2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r +
                            5.46378491116411436990e+0) * r + 6.65790464350110377720e+0;
        const double den = ((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
                               7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
                            5.99832206555887937690e-1) * r + 1.0;
        x = num / den;
    }
    return q < 0.0 ? -x : x;
}

// rules 7 and 8: count / n clipped to [1 / (2 n), 1 - 1 / (2 n)]
__device__ __forceinline__ double npde_clipped(int count, int n) {
    const double lo = 1.0 / (2.0 * (double)n), hi = 1.0 - lo;
    const double p = (double)count / (double)n;
    return p < lo ? lo : (p > hi ? hi : p);
}

__global__ __launch_bounds__(kNpdeThreads) void npde_place_kernel(NpdePlaceArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kNpdeThreads + threadIdx.x;
    if (i >= a.N) return;
    const int k = blockIdx.y;
    const double z = rng_npde_normal(a.seed, a.subject_offset + i, a.first_rep + k, kRngKindNpdeEta);
    a.out[(int64_t)k * a.N + i] = a.normals_only ? z : npde_effect(a.prior_mean, a.prior_sd, z);
}

__global__ __launch_bounds__(kNpdeThreads) void npde_observe_kernel(NpdeObserveArgs a) {
    const int64_t li = (int64_t)blockIdx.x * kNpdeThreads + threadIdx.x;
    if (li >= a.n_subj) return;
    const int k = blockIdx.y, R = a.T - 1;
    const int64_t i = a.subj0 + li;
    double* const y = a.y + (int64_t)k * R * a.n_subj + li;
    if (a.noise_only) {
        for (int r = 0; r < R; r++)
            y[(int64_t)r * a.n_subj] = rng_npde_normal(a.seed, a.subject_offset + i, a.first_rep + k, kRngKindNpdeNoise | (uint32_t)r);
        return;
    }
    const double* const v = a.slab + ((int64_t)k * a.n_subj + li) * ((int64_t)a.T * a.NS) + a.state;
    const double sigma = a.sigma[i];
    bool ok = true;
    for (int r = 0; r < R; r++) {
        const double eps = a.from_noise ? y[(int64_t)r * a.n_subj]
                                        : rng_npde_normal(a.seed, a.subject_offset + i, a.first_rep + k, kRngKindNpdeNoise | (uint32_t)r);
        const double ys = simulated_observation(v[(int64_t)(r + 1) * a.NS], sigma, a.scale, eps);      // rule 4
        y[(int64_t)r * a.n_subj] = ys;
        ok = ok && finite_value(ys);
    }
    a.used[(int64_t)k * a.n_subj + li] = ok ? 1 : 0;
}

// RMAX: the rows the substitution's register arrays are unrolled for (R <= RMAX; 8, 16 or 31 -- 255 VGPRs at 31)
template <int RMAX>
__global__ __launch_bounds__(kNpdeThreads) void npde_reduce_kernel(NpdeReduceArgs a, int C) {
    extern __shared__ double s_d[];
    const int tid = threadIdx.x;
    const int R = a.R, K = a.K, E = R * (R + 1) / 2;
    double* const s_m = s_d;                          // [R][C]
    double* const s_L = s_m + R * C;                  // [E][C]: C, then L
    double* const s_w = s_L + E * C;                  // [R][C]: y_obs, then w_obs
    int32_t* const s_cnt = (int32_t*)(s_w + R * C);   // [R][C]: rule 8's counts
    int32_t* const s_n = s_cnt + R * C;               // [C]
    int32_t* const s_st = s_n + C;                    // [C]
    const int64_t q0 = (int64_t)blockIdx.x * C;       // first subject of the tile, inside the pass
    const int nc = (int)(a.n_subj - q0 < C ? a.n_subj - q0 : C);
    const int64_t n_subj = a.n_subj;
    const double nan = __builtin_nan("");
    // ---- the observation; BAD_OBS
    for (int idx = tid; idx < R * C; idx += kNpdeThreads) {
        const int r = idx / C, cc = idx - r * C;
        s_w[idx] = cc < nc ? a.obs[(int64_t)(r + 1) * a.N + a.subj0 + q0 + cc] : 0.0;
        s_cnt[idx] = 0;
    }
    __syncthreads();
    if (tid < C) {
        int32_t st = 0;
        if (tid < nc) {
            bool ok = finite_value(a.sigma[a.subj0 + q0 + tid]);
            for (int r = 0; r < R; r++) ok = ok && finite_value(s_w[r * C + tid]);
            if (!ok) st = kNpdeBadObs;
        }
        s_st[tid] = st;
    }
    __syncthreads();
    // ---- rules 5 ... 7, one lane per (row, subject), in replicate order
    for (int idx = tid; idx < R * C; idx += kNpdeThreads) {
        const int r = idx / C, cc = idx - r * C;
        if (cc >= nc) continue;
        const int64_t q = q0 + cc;
        const bool bad = s_st[cc] != 0;
        const double yobs = s_w[idx];
        const uint8_t* const used = a.used + q;
        const double* const y = a.y + (int64_t)r * n_subj + q;
        int n = 0, below = 0;
        double sum = 0.0;
        // (branch-free, so that the loads of several simulations are in flight at once: the adds stay in replicate order)
#pragma unroll 8
        for (int k = 0; k < K; k++) {
            const double v = y[(int64_t)k * R * n_subj];
            const bool u = used[(int64_t)k * n_subj] != 0;
            n += u ? 1 : 0;
            sum = u ? sum + v : sum;
            below += (u && v < yobs) ? 1 : 0;
        }
        const double m = sum / (double)n;
        s_m[idx] = m;
        if (r == 0) s_n[cc] = n;
        const int64_t o = (int64_t)r * a.N + a.subj0 + q;
        if (a.pred_mean) a.pred_mean[o] = bad ? nan : m;
        if (a.below) a.below[o] = bad ? -1 : below;
        if (a.pd) a.pd[o] = bad ? nan : npde_clipped(below, n);
    }
    __syncthreads();
    // ---- rule 6's C, one lane per (triangle entry, subject)
    for (int idx = tid; idx < E * C; idx += kNpdeThreads) {
        const int e = idx / C, cc = idx - e * C;
        if (cc >= nc) continue;
        int r = 0;
        while ((r + 1) * (r + 2) / 2 <= e) r++;
        const int s = e - r * (r + 1) / 2;
        const int64_t q = q0 + cc;
        const double mr = s_m[r * C + cc], ms = s_m[s * C + cc];
        const uint8_t* const used = a.used + q;
        const double* const yr = a.y + (int64_t)r * n_subj + q;
        const double* const ys = a.y + (int64_t)s * n_subj + q;
        double acc = 0.0;
#pragma unroll 8
        for (int k = 0; k < K; k++) {
            const double vr = yr[(int64_t)k * R * n_subj], vs = ys[(int64_t)k * R * n_subj];
            const double next = npde_cross_add(acc, vr, mr, vs, ms);
            acc = used[(int64_t)k * n_subj] ? next : acc;
        }
        const double c = acc / (double)(s_n[cc] - 1);
        s_L[idx] = c;
        if (s == r && a.pred_var) a.pred_var[(int64_t)r * a.N + a.subj0 + q] = s_st[cc] != 0 ? nan : c;
    }
    __syncthreads();
    // ---- rule 8's factor and w_obs, one lane per subject
    if (tid < nc) {
        const int cc = tid;
        const int n = s_n[cc];
        int32_t st = s_st[cc];
        if (st == 0) {
            if (n < K) st |= kNpdeFailedSims;
            if (n <= R) st |= kNpdeFew;
            else {
                for (int r = 0; r < R && !(st & kNpdeSingular); r++) {
                    const int er = r * (r + 1) / 2;
                    for (int s = 0; s < r; s++) {
                        const int es = s * (s + 1) / 2;
                        double acc = s_L[(er + s) * C + cc];
                        for (int j = 0; j < s; j++) acc = npde_mul_sub(acc, s_L[(er + j) * C + cc], s_L[(es + j) * C + cc]);
                        s_L[(er + s) * C + cc] = acc / s_L[(es + s) * C + cc];
                    }
                    const double crr = s_L[(er + r) * C + cc];
                    double p = crr;
                    for (int j = 0; j < r; j++) {
                        const double l = s_L[(er + j) * C + cc];
                        p = npde_mul_sub(p, l, l);
                    }
                    if (!(p > kNpdePivotTol * crr)) st |= kNpdeSingular;
                    s_L[(er + r) * C + cc] = sqrt(p);
                }
                if (!(st & kNpdeSingular)) {
                    for (int r = 0; r < R; r++) {
                        const int er = r * (r + 1) / 2;
                        double acc = s_w[r * C + cc] - s_m[r * C + cc];
                        for (int j = 0; j < r; j++) acc = npde_mul_sub(acc, s_L[(er + j) * C + cc], s_w[j * C + cc]);
                        s_w[r * C + cc] = acc / s_L[(er + r) * C + cc];
                    }
                }
            }
        }
        s_st[cc] = st;
        const int64_t i = a.subj0 + q0 + cc;
        if (a.status) a.status[i] = st;
        if (a.n_used) a.n_used[i] = (st & kNpdeBadObs) ? -1 : n;
        if ((st & (kNpdeSingular | kNpdeFew | kNpdeBadObs)) && a.n_failed) atomicAdd(a.n_failed, 1);
    }
    __syncthreads();
    // ---- rule 8's substitution: G lanes per subject, lane g takes simulations g, g + G, ...; w and the counts in registers
    if (a.below_decorr || a.npde) {
        const int G = kNpdeThreads / C;
        const int cc = tid % C, g = tid / C;
        if (g < G && cc < nc && !(s_st[cc] & (kNpdeSingular | kNpdeFew | kNpdeBadObs))) {
            const int64_t q = q0 + cc;
            int32_t cnt[RMAX];
#pragma unroll
            for (int r = 0; r < RMAX; r++) cnt[r] = 0;
            for (int k = g; k < K; k += G) {
                if (!a.used[(int64_t)k * n_subj + q]) continue;
                const double* const y = a.y + (int64_t)k * R * n_subj + q;
                double w[RMAX];
#pragma unroll
                for (int r = 0; r < RMAX; r++) {
                    if (r < R) {
                        double acc = y[(int64_t)r * n_subj] - s_m[r * C + cc];
#pragma unroll
                        for (int j = 0; j < r; j++) acc = npde_mul_sub(acc, s_L[(r * (r + 1) / 2 + j) * C + cc], w[j]);
                        w[r] = acc / s_L[(r * (r + 1) / 2 + r) * C + cc];
                        cnt[r] += w[r] < s_w[r * C + cc] ? 1 : 0;
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < RMAX; r++)
                if (r < R && cnt[r]) atomicAdd(&s_cnt[r * C + cc], cnt[r]);
        }
        __syncthreads();
        for (int idx = tid; idx < R * C; idx += kNpdeThreads) {
            const int r = idx / C, cc = idx - r * C;
            if (cc >= nc) continue;
            const bool none = (s_st[cc] & (kNpdeSingular | kNpdeFew | kNpdeBadObs)) != 0;
            const int64_t o = (int64_t)r * a.N + a.subj0 + q0 + cc;
            if (a.below_decorr) a.below_decorr[o] = none ? -1 : s_cnt[idx];
            if (a.npde) a.npde[o] = none ? nan : npde_ppnd16(npde_clipped(s_cnt[idx], s_n[cc]));
        }
    }
}

// subjects of a tile and its LDS: m, the triangle, w (doubles), the counts (int32) per row; n_used and status per subject
int npde_tile(int R, size_t* lds) {
    const size_t per = 8 * (size_t)(R * (R + 5) / 2) + 4 * (size_t)R + 8;
    const int C = (int)std::min<size_t>(kNpdeMaxCols, kNpdeTileBytes / per);
    *lds = per * (size_t)C;
    return C;
}
}  // namespace

hipError_t launch_npde_place(const NpdePlaceArgs& a, hipStream_t s) {
    if (a.N < 1 || a.K < 1 || a.K > kPredMaxSets || a.first_rep < 0 || a.first_rep + a.K > kRngMaxReplicate || !a.out)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(npde_place_kernel, dim3((unsigned)((a.N + kNpdeThreads - 1) / kNpdeThreads), (unsigned)a.K),
                       dim3(kNpdeThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_npde_observe(const NpdeObserveArgs& a, hipStream_t s) {
    if (a.n_subj < 1 || a.subj0 < 0 || a.K < 1 || a.K > kPredMaxSets || a.T < 2 || a.T > kMaxObs || !a.y || a.first_rep < 0 ||
        a.first_rep + a.K > kRngMaxReplicate)
        return hipErrorInvalidValue;
    if (!a.noise_only && (!a.slab || !a.sigma || !a.used || a.NS < 1 || a.state < 0 || a.state >= a.NS)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(npde_observe_kernel, dim3((unsigned)((a.n_subj + kNpdeThreads - 1) / kNpdeThreads), (unsigned)a.K),
                       dim3(kNpdeThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_npde_reduce(const NpdeReduceArgs& a, hipStream_t s) {
    if (a.n_subj < 1 || a.subj0 < 0 || a.subj0 + a.n_subj > a.N || a.K < 2 || a.K > kPredMaxSets || a.R < 1 ||
        a.R > kNpdeMaxRows || !a.y || !a.used || !a.obs || !a.sigma)
        return hipErrorInvalidValue;
    size_t lds = 0;
    const int C = npde_tile(a.R, &lds);
    const int64_t tiles = (a.n_subj + C - 1) / C;
    const dim3 grid((unsigned)tiles), block(kNpdeThreads);
    if (a.R <= 8) hipLaunchKernelGGL(npde_reduce_kernel<8>, grid, block, lds, s, a, C);
    else if (a.R <= 16) hipLaunchKernelGGL(npde_reduce_kernel<16>, grid, block, lds, s, a, C);
    else hipLaunchKernelGGL(npde_reduce_kernel<kNpdeMaxRows>, grid, block, lds, s, a, C);
    return hipGetLastError();
}

}  // namespace cude
