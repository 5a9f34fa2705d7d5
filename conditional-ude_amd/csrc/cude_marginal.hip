// Per-subject marginal likelihoods (cude_marginal_likelihood; the numbered rules in include/cude.h): the integration points
// of every subject are placed on the device, and every chunk of their SSEs -- left by the multi-set forward launch where
// it wrote them -- is folded into a running, rescaled log-sum per subject.
//
// Stands for (reference repo paths): the integral over eta of exp(individual_log_likelihood + logpdf(Normal(prior_mean,
// prior_sd), eta)), src/saem.jl:55-66, i.e. of exp(-map_objective), src/saem-symreg.jl:68-73.
//
// Layout: points, draws, SSEs and terms are [k][N] rows, so one lane per subject reads every row as one coalesced 512-byte
// segment per wave; the six-double state is [6][N] for the same reason.  A subject's nodes are folded in strictly in node
// order by ONE lane, whatever the chunk size: nothing is reduced across lanes, so no output depends on the decomposition.
// The arithmetic is a few dozen flops and one exp per node and subject beside a whole ODE solve: the kernels are sized for
// occupancy of the memory system (64-wide workgroups, one wave each: N = 117 still spreads over two compute units), not
// tuned further.
//
// Every expression is rounded operation by operation (contraction off): the points have numpy's bits (rule 1), and the
// sums do not depend on what the compiler fuses.
#include <hip/hip_runtime.h>

#include "cude_kernels.h"
#include "cude_rng.h"

namespace cude {

namespace {
constexpr int kMarginalThreads = 64;
constexpr double kHalfLog2Pi = 0.91893853320467274178;
constexpr double kDblMax = 1.79769313486231570815e308;

__device__ __forceinline__ bool is_finite(double v) { return fabs(v) <= kDblMax; }

// rule 1: x = center + scale z, the product rounded, then the sum
__device__ __forceinline__ double marginal_point(double center, double scale, double z) {
#pragma clang fp contract(off)
    const double p = scale * z;
    return center + p;
}

// rule 1.  grid: x over the subjects, y over the chunk's rows
__global__ __launch_bounds__(kMarginalThreads) void marginal_points_kernel(MarginalArgs a, int k0, double* __restrict__ x,
                                                                           double* __restrict__ z) {
    const int64_t i = (int64_t)blockIdx.x * kMarginalThreads + threadIdx.x;
    if (i >= a.N) return;
    const int k = blockIdx.y;
    const int64_t r = (int64_t)k * a.N + i;
    double zk;
    if (a.nodes != nullptr) {
        zk = a.nodes[k0 + k];
    } else {
        zk = rng_normal(RngKey{a.key.seed, a.key.subject_offset, a.key.step + k0 + k}, i);
        z[r] = zk;
    }
    x[r] = marginal_point(a.center[i], a.scale != nullptr ? a.scale[i] : 1.0, zk);
}

// rules 2 and 3: one lane per subject walks the chunk's rows in node order
__global__ __launch_bounds__(kMarginalThreads) void marginal_accumulate_kernel(MarginalArgs a, int k0, int kn,
                                                                               const double* __restrict__ sse,
                                                                               const double* __restrict__ x,
                                                                               const double* __restrict__ z,
                                                                               double* __restrict__ terms) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kMarginalThreads + threadIdx.x;
    if (i >= a.N) return;
    const int64_t N = a.N;
    const double ninf = -__builtin_huge_val();
    double M = ninf, S0 = 0.0, S1 = 0.0, S2 = 0.0, S3 = 0.0, Q = 0.0;
    int32_t n_bad = 0;
    if (k0 > 0) {
        M = a.state[i]; S0 = a.state[N + i]; S1 = a.state[2 * N + i]; S2 = a.state[3 * N + i]; S3 = a.state[4 * N + i];
        Q = a.state[5 * N + i];
        n_bad = a.n_bad[i];
    }
    const double sc = a.scale != nullptr ? a.scale[i] : 1.0;
    const bool subject_ok = is_finite(a.center[i]) && is_finite(sc) && sc > 0.0;
    const bool prior = a.prior_sd < __builtin_huge_val();
    for (int k = 0; k < kn; k++) {
        const int64_t r = (int64_t)k * N + i;
        const double s = sse[r], xk = x[r];
        double zk, ak;
        if (a.nodes != nullptr) {
            zk = a.nodes[k0 + k];
            ak = a.log_weights[k0 + k];
        } else {
            zk = z[r];
            ak = a.c_K + 0.5 * (zk * zk);
        }
        double t = ninf;
        if (subject_ok && is_finite(s)) {
            const double ll = fma(-s, a.inv_2s2, a.ll_const);
            double lp = 0.0;
            if (prior) {
                const double u = (xk - a.prior_mean) / a.prior_sd;
                lp = (-0.5 * (u * u) - a.log_prior_sd) - kHalfLog2Pi;
            }
            t = (ak + ll) + lp;
            if (!is_finite(t)) t = ninf;
        }
        if (terms != nullptr) terms[r] = t;
        if (!(t > ninf)) { n_bad++; continue; }
        double e;
        if (t > M) {
            const double rr = exp(M - t);
            S0 = S0 * rr; S1 = S1 * rr; S2 = S2 * rr; S3 = S3 * rr;
            Q = Q * (rr * rr);
            M = t;
            e = 1.0;
        } else {
            e = exp(t - M);
        }
        S0 = S0 + e;
        S1 = S1 + e * zk;
        S2 = S2 + e * (zk * zk);
        S3 = S3 + e * s;
        Q = Q + e * e;
    }
    a.state[i] = M; a.state[N + i] = S0; a.state[2 * N + i] = S1; a.state[3 * N + i] = S2; a.state[4 * N + i] = S3;
    a.state[5 * N + i] = Q;
    a.n_bad[i] = n_bad;
}

// rule 4
__global__ __launch_bounds__(kMarginalThreads) void marginal_finish_kernel(MarginalArgs a, double* __restrict__ logml,
                                                                           double* __restrict__ post_mean,
                                                                           double* __restrict__ post_var,
                                                                           double* __restrict__ post_sse,
                                                                           double* __restrict__ ess,
                                                                           int32_t* __restrict__ n_failed) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kMarginalThreads + threadIdx.x;
    if (i >= a.N) return;
    const int64_t N = a.N;
    const double nan = __builtin_nan("");
    double lm = -__builtin_huge_val(), pm = nan, pv = nan, ps = nan, es = nan;
    if (a.n_bad[i] < a.n_nodes) {
        const double M = a.state[i], S0 = a.state[N + i], S1 = a.state[2 * N + i], S2 = a.state[3 * N + i],
                     S3 = a.state[4 * N + i], Q = a.state[5 * N + i];
        const double c = a.center[i], sc = a.scale != nullptr ? a.scale[i] : 1.0;
        const double m1 = S1 / S0, m2 = S2 / S0;
        const double v = m2 - m1 * m1;
        lm = (M + log(S0)) + log(sc);
        pm = c + sc * m1;
        pv = (sc * sc) * (v > 0.0 ? v : 0.0);
        ps = S3 / S0;
        es = (S0 * S0) / Q;
    } else {
        atomicAdd(n_failed, 1);
    }
    if (logml != nullptr) logml[i] = lm;
    if (post_mean != nullptr) post_mean[i] = pm;
    if (post_var != nullptr) post_var[i] = pv;
    if (post_sse != nullptr) post_sse[i] = ps;
    if (ess != nullptr) ess[i] = es;
}

inline unsigned subject_blocks(int64_t N) { return (unsigned)((N + kMarginalThreads - 1) / kMarginalThreads); }
}  // namespace

hipError_t launch_marginal_points(const MarginalArgs& a, int k0, int kn, double* x, double* z, hipStream_t s) {
    hipLaunchKernelGGL(marginal_points_kernel, dim3(subject_blocks(a.N), (unsigned)kn), dim3(kMarginalThreads), 0, s, a, k0, x, z);
    return hipGetLastError();
}

hipError_t launch_marginal_accumulate(const MarginalArgs& a, int k0, int kn, const double* sse, const double* x, const double* z,
                                      double* terms, hipStream_t s) {
    hipLaunchKernelGGL(marginal_accumulate_kernel, dim3(subject_blocks(a.N)), dim3(kMarginalThreads), 0, s, a, k0, kn, sse, x, z,
                       terms);
    return hipGetLastError();
}

hipError_t launch_marginal_finish(const MarginalArgs& a, double* logml, double* post_mean, double* post_var, double* post_sse,
                                  double* ess, int32_t* n_failed, hipStream_t s) {
    hipLaunchKernelGGL(marginal_finish_kernel, dim3(subject_blocks(a.N)), dim3(kMarginalThreads), 0, s, a, logml, post_mean,
                       post_var, post_sse, ess, n_failed);
    return hipGetLastError();
}

}  // namespace cude
