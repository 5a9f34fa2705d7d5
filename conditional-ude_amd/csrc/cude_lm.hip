// libcude_hip.so -- Levenberg-Marquardt on the expected-information matrices (cude_lm_candidates, cude_train_lm; the numbered
// rules in include/cude.h).  One gradient launch leaves the half-gradients, the information pass of cude_batch.hip
// (info_pass) leaves A, b_i, d_i and the status on the device; the kernels here turn them into K damped steps at once:
//
//   scale       M_theta, M_c and their maxima, ghat = (N / 2) g, the max-norm of g (one workgroup)
//   tables      t_i^k = b_i / sqrt(e_i^k), e_i^k = d_i + mu_k M_c,i; the Schur sums sum_i t_i^k t_i^k^T are
//               cude_jacobian.hip's cross kernel on table k (blocks of 1024 subjects in index order)
//   rhs         sum_i b_i ghat_c,i / e_i^k: one workgroup per (parameter, k), 256 strided sums and a halving tree
//   cholesky    one workgroup per k, one lane per row, left-looking; S_mu in LDS when it fits (P <= kLmLdsP), else in device
//               memory; then the two triangular solves
//   candidates  one lane per (subject, k): delta c_i, the trial sets in eval_sets_device's layout, the subject's term of pred
//   pred        per k: the terms in the rhs kernel's order, then the parameters' terms in index order
//   losses      the trial losses in cude_multistart_forward's arithmetic
//   select      one lane: the lowest finite trial loss below the current one, ties to the lower index
//   commit      the selected set into the context's parameters
#include "cude_ctx.h"

using namespace cude::api;

namespace {
constexpr int kLmThreads = 256;
constexpr int kLmMaxK = 8;
constexpr int kLmMaxP = 193;                      // the largest tuned shape; one lane per row of S_mu
constexpr int kLmLdsP = 86;                       // 8 (P^2 + P) bytes <= 60 KB
constexpr double kLmFloor = 1e-8;
constexpr double kLmRatio = 5.0;                  // between the rungs of the damping ladder (include/cude.h rule 9)
constexpr double kLmMuMin = 1e-15, kLmMuMax = 1e15;
constexpr double kDblMax = 1.79769313486231570815e308;

struct LmArgs {
    int64_t N;
    int32_t P, K, use_lds;
    double mu[kLmMaxK];
    double n_lambda, half_n, n_global, lambda;
    const double *A, *b, *d, *mask, *g_nn, *g_cond, *nn, *cond;
    const int32_t *status, *nfail;
    double *gth, *gc, *Mth, *Mc, *tab, *X, *rvec, *work, *dth, *nn_sets, *cond_sets, *term, *pred, *sums, *loss, *rec, *part, *dcond;
    int32_t* valid;
};

__device__ __forceinline__ bool lm_finite(double v) { return fabs(v) <= kDblMax; }
__device__ __forceinline__ bool lm_off(const double* __restrict__ mask, int q) { return mask != nullptr && mask[q] == 0.0; }
// e_i^k = d_i + mu_k M_c,i, the product and the sum rounded on their own: the same bits in every kernel that forms it
__device__ __forceinline__ double lm_e(double d, double mu, double mc) {
#pragma clang fp contract(off)
    const double m = mu * mc;
    return d + m;
}
// the workgroup's 256 values by the halving tree; the result in every lane
__device__ __forceinline__ double lm_tree_sum(double v, double* s) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (int off = kLmThreads / 2; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ double lm_tree_max(double v, double* s) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (int off = kLmThreads / 2; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) s[threadIdx.x] = fmax(s[threadIdx.x], s[threadIdx.x + off]);
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}

// one workgroup.  rec[0] = max-norm of the loss gradient (NaN if an entry is), rec[1] = failed subjects of the gradient
// launch, rec[2] = failed subjects of the information pass
__global__ __launch_bounds__(kLmThreads) void lm_scale_kernel(LmArgs a) {
    __shared__ double s[kLmThreads];
    const int P = a.P;
    const int64_t N = a.N;
    double ma = 0.0, md = 0.0, mg = 0.0;
    bool bad = false;
    for (int q = threadIdx.x; q < P; q += kLmThreads) {
        ma = fmax(ma, a.A[(int64_t)q * P + q] + a.n_lambda);
        const double g = a.g_nn[q];
        bad |= !lm_finite(g);
        mg = fmax(mg, fabs(g));
    }
    for (int64_t i = threadIdx.x; i < N; i += kLmThreads) {
        md = fmax(md, a.d[i]);
        const double g = a.g_cond[i];
        bad |= !lm_finite(g);
        mg = fmax(mg, fabs(g));
    }
    ma = lm_tree_max(ma, s);
    md = lm_tree_max(md, s);
    mg = lm_tree_max(mg, s);
    const double nbad = lm_tree_sum(bad ? 1.0 : 0.0, s);
    const double fa = kLmFloor * ma, fd = kLmFloor * md;
    for (int q = threadIdx.x; q < P; q += kLmThreads) {
        a.Mth[q] = ma > 0.0 ? fmax(a.A[(int64_t)q * P + q] + a.n_lambda, fa) : 1.0;
        a.gth[q] = a.half_n * a.g_nn[q];
    }
    for (int64_t i = threadIdx.x; i < N; i += kLmThreads) {
        a.Mc[i] = md > 0.0 ? fmax(a.d[i], fd) : 1.0;        // (fmax: the floor for a failed subject's NaN)
        a.gc[i] = a.half_n * a.g_cond[i];
    }
    if (threadIdx.x == 0) {
        a.rec[0] = nbad > 0.0 ? __builtin_nan("") : mg;
        a.rec[1] = a.g_nn[P + 1];
        a.rec[2] = (double)*a.nfail;
    }
}

// grid: x over the subjects, y over the parameters, z over the dampings
__global__ __launch_bounds__(kLmThreads) void lm_tables_kernel(LmArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kLmThreads + threadIdx.x;
    if (i >= a.N) return;
    const int q = blockIdx.y, k = blockIdx.z;
    const double e = lm_e(a.d[i], a.mu[k], a.Mc[i]);
    a.tab[((int64_t)k * a.P + q) * a.N + i] = a.b[(int64_t)q * a.N + i] / sqrt(e);
}

// grid: x over the parameters, y over the dampings
__global__ __launch_bounds__(kLmThreads) void lm_rhs_kernel(LmArgs a) {
    __shared__ double s[kLmThreads];
    const int q = blockIdx.x, k = blockIdx.y;
    const int64_t N = a.N;
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += kLmThreads) {
#pragma clang fp contract(off)
        const double t = a.b[(int64_t)q * N + i] * a.gc[i];
        v += t / lm_e(a.d[i], a.mu[k], a.Mc[i]);
    }
    v = lm_tree_sum(v, s);
    if (threadIdx.x == 0) a.rvec[(int64_t)k * a.P + q] = v;
}

// grid: x over the dampings; one lane per row.  Dynamic LDS: [P] doubles, and [P][P] with use_lds.
__global__ __launch_bounds__(kLmThreads) void lm_cholesky_kernel(LmArgs a) {
    extern __shared__ double lds[];
    __shared__ double s_piv;
    __shared__ int s_bad;
    const int P = a.P, k = blockIdx.x, i = threadIdx.x;
    const double mu = a.mu[k];
    double* const v = lds;
    double* const S = a.use_lds ? lds + P : a.work + (int64_t)k * P * P;
    const double* const X = a.X + (int64_t)k * P * P;
    const bool row = i < P;
    const bool off_i = row && lm_off(a.mask, i);
    if (i == 0) s_bad = *a.nfail > 0 ? 1 : 0;
    if (row) {
        // the lower triangle of S_mu, row i: (A + N lambda I + mu M) - sum_i t t^T; a masked row / column: the unit diagonal
        for (int r = 0; r <= i; r++) {
#pragma clang fp contract(off)
            double sv;
            if (off_i || lm_off(a.mask, r)) {
                sv = r == i ? 1.0 : 0.0;
            } else {
                double h = a.A[(int64_t)i * P + r];
                if (r == i) {
                    const double m = mu * a.Mth[i];
                    h = (h + a.n_lambda) + m;
                }
                sv = h - X[(int64_t)i * P + r];
            }
            S[(int64_t)i * P + r] = sv;
        }
        double rv = 0.0;
        if (!off_i) {
#pragma clang fp contract(off)
            rv = -(a.gth[i] - a.rvec[(int64_t)k * P + i]);
        }
        v[i] = rv;
    }
    __syncthreads();
    for (int j = 0; j < P; j++) {
        double sv = 0.0;
        if (row && i >= j) {
            sv = S[(int64_t)i * P + j];
            for (int c = 0; c < j; c++) sv = fma(-S[(int64_t)i * P + c], S[(int64_t)j * P + c], sv);
            if (i == j) s_piv = sv;
        }
        __syncthreads();
        const double piv = s_piv;
        if (!(piv > 0.0) || !lm_finite(piv)) {          // (the same value in every lane: they leave together)
            if (i == 0) s_bad = 1;
            break;
        }
        const double l = sqrt(piv);
        if (row && i == j) S[(int64_t)i * P + j] = l;
        if (row && i > j) S[(int64_t)i * P + j] = sv / l;
        __syncthreads();
    }
    __syncthreads();
    if (s_bad == 0) {
        for (int j = 0; j < P; j++) {                   // L y = rhs
            if (i == j) v[j] = v[j] / S[(int64_t)j * P + j];
            __syncthreads();
            if (row && i > j) v[i] = fma(-S[(int64_t)i * P + j], v[j], v[i]);
            __syncthreads();
        }
        for (int j = P - 1; j >= 0; j--) {              // L^T x = y
            if (i == j) v[j] = v[j] / S[(int64_t)j * P + j];
            __syncthreads();
            if (row && i < j) v[i] = fma(-S[(int64_t)j * P + i], v[j], v[i]);
            __syncthreads();
        }
        if (row && !lm_finite(v[i])) s_bad = 1;
    }
    __syncthreads();
    const bool ok = s_bad == 0;
    if (row) a.dth[(int64_t)k * P + i] = !ok ? __builtin_nan("") : (off_i ? 0.0 : v[i]);
    if (i == 0) a.valid[k] = ok ? 1 : 0;
}

// grid: x over the subjects, y over the dampings
__global__ __launch_bounds__(kLmThreads) void lm_candidates_kernel(LmArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kLmThreads + threadIdx.x;
    const int k = blockIdx.y, P = a.P;
    const int64_t N = a.N;
    const bool ok = a.valid[k] != 0;
    const double* const dth = a.dth + (int64_t)k * P;
    // (an invalid candidate's trial set is the current point: its solve is spent, its loss is NaN afterwards)
    if (blockIdx.x == 0)
        for (int q = threadIdx.x; q < P; q += kLmThreads)
            a.nn_sets[(int64_t)k * P + q] = (!ok || lm_off(a.mask, q)) ? a.nn[q] : a.nn[q] + dth[q];
    if (i >= N) return;
    double dc = 0.0, term = 0.0;
    if (ok) {
#pragma clang fp contract(off)
        double s = 0.0;
        for (int q = 0; q < P; q++) s = fma(a.b[(int64_t)q * N + i], dth[q], s);
        const double e = lm_e(a.d[i], a.mu[k], a.Mc[i]);
        dc = -(a.gc[i] + s) / e;
        const double t1 = a.gc[i] * dc;
        const double t2 = (a.mu[k] * a.Mc[i]) * (dc * dc);
        term = t2 - t1;
    }
    a.cond_sets[(int64_t)k * N + i] = ok ? a.cond[i] + dc : a.cond[i];
    a.dcond[(int64_t)k * N + i] = ok ? dc : __builtin_nan("");
    a.term[(int64_t)k * N + i] = term;
}

// grid: x over the dampings.  pred_k = -ghat^T delta + mu delta^T M delta
__global__ __launch_bounds__(kLmThreads) void lm_pred_kernel(LmArgs a) {
    __shared__ double s[kLmThreads];
    const int k = blockIdx.x, P = a.P;
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < a.N; i += kLmThreads) v += a.term[(int64_t)k * a.N + i];
    v = lm_tree_sum(v, s);
    if (threadIdx.x != 0) return;
    if (!a.valid[k]) { a.pred[k] = __builtin_nan(""); return; }
    for (int q = 0; q < P; q++) {
#pragma clang fp contract(off)
        const double dq = a.dth[(int64_t)k * P + q];
        const double t1 = a.gth[q] * dq;
        const double t2 = (a.mu[k] * a.Mth[q]) * (dq * dq);
        v += t2 - t1;
    }
    a.pred[k] = v;
}

// one lane per damping: sums [K][2] = (sum SSE, failures) -> the loss value in cude_multistart_forward's arithmetic
__global__ void lm_losses_kernel(LmArgs a) {
#pragma clang fp contract(off)
    const int k = threadIdx.x;
    if (k >= a.K) return;
    if (!a.valid[k]) { a.loss[k] = __builtin_nan(""); return; }
    double reg = 0.0;
    if (a.lambda != 0.0)
        for (int q = 0; q < a.P; q++) {
            const double w = a.nn_sets[(int64_t)k * a.P + q];
            const double w2 = w * w;
            reg += w2;
        }
    const double sum = a.sums[2 * k], nf = a.sums[2 * k + 1];
    const double t1 = sum / a.n_global, t2 = a.lambda * reg;
    a.loss[k] = (nf > 0.0 || !lm_finite(sum)) ? __builtin_inf() : t1 + t2;
}

// one lane: rec[3] = the selected candidate (-1: none), rec[4] = its trial loss
__global__ void lm_select_kernel(LmArgs a, double f_cur) {
    int best = -1;
    double fb = f_cur;
    for (int k = 0; k < a.K; k++) {
        const double f = a.loss[k];
        if (lm_finite(f) && f < fb) { fb = f; best = k; }
    }
    a.rec[3] = (double)best;
    a.rec[4] = best < 0 ? __builtin_nan("") : fb;
}

__global__ __launch_bounds__(kLmThreads) void lm_commit_kernel(LmArgs a, double* __restrict__ nn, double* __restrict__ cond) {
    const int sel = (int)a.rec[3];
    if (sel < 0) return;
    const int64_t e = (int64_t)blockIdx.x * kLmThreads + threadIdx.x;
    if (e < a.P) nn[e] = a.nn_sets[(int64_t)sel * a.P + e];
    else if (e < a.P + a.N) cond[e - a.P] = a.cond_sets[(int64_t)sel * a.N + (e - a.P)];
}

unsigned lm_blocks(int64_t n) { return (unsigned)((n + kLmThreads - 1) / kLmThreads); }

// mu_k = mu 5^(k - 1), k = 0 ... K - 1
void lm_ladder(double mu, int K, double* out) {
    out[0] = mu / kLmRatio;
    double f = 1.0;
    for (int k = 1; k < K; k++) { out[k] = mu * f; f *= kLmRatio; }
}

int32_t lm_check_state(cude_ctx* c, const char* who) {
    if (!c->have_pop) return fail(CUDE_ERR_STATE, "population not set");
    if (!c->have_nn || !c->have_cond) return fail(CUDE_ERR_STATE, "parameters not set");
    if (c->capturing) return fail(CUDE_ERR_STATE, std::string(who) + " under stream capture");
    if (distributed(c)) return fail(CUDE_ERR_UNSUPPORTED, std::string(who) + ": a sharded population is not supported");
    if (c->P > kLmMaxP) return fail(CUDE_ERR_UNSUPPORTED, std::string(who) + ": more than 193 shared parameters");
    return CUDE_OK;
}

// Scratch for K dampings and the argument record (everything but mu).
int32_t lm_setup(cude_ctx* c, int K, LmArgs& a, double** nn_bak, double** cond_bak) {
    const int P = c->P;
    const int64_t N = c->N;
    a = LmArgs{};
    a.N = N; a.P = P; a.K = K; a.use_lds = P <= kLmLdsP ? 1 : 0;
    a.n_global = c->n_global; a.lambda = c->cfg.lambda;
    a.n_lambda = c->n_global * c->cfg.lambda;
    a.half_n = 0.5 * c->n_global;
    const size_t n_part = cude::info_cross_partials(N, P);
    HIP_TRY(carve(c->lm_buf, [&](Carve<double>& v) {
        a.gth = v.take(P); a.gc = v.take(N); a.Mth = v.take(P); a.Mc = v.take(N);
        a.tab = v.take((size_t)K * P * N);
        a.part = v.take(n_part);
        a.X = v.take((size_t)K * P * P);
        a.rvec = v.take((size_t)K * P);
        a.work = v.take((size_t)K * P * P);
        a.dth = v.take((size_t)K * P);
        a.nn_sets = v.take((size_t)K * P);
        a.cond_sets = v.take((size_t)K * N);
        a.term = v.take((size_t)K * N);
        a.dcond = v.take((size_t)K * N);
        a.pred = v.take(K); a.sums = v.take((size_t)2 * K); a.loss = v.take(K); a.rec = v.take(8);
        *nn_bak = v.take(P); *cond_bak = v.take(N);
    }));
    HIP_TRY(c->lm_int.reserve((size_t)K));
    a.valid = c->lm_int.p;
    a.mask = c->param_mask.p;
    a.g_nn = c->g_nn.p; a.g_cond = c->g_cond.p; a.nn = c->nn.p; a.cond = c->cond.p;
    return CUDE_OK;
}

// One gradient launch, one information pass and the K damped steps and trial losses at the context's parameters, all
// queued on its stream.  Leaves the trial sets, pred, loss, valid and rec[0 ... 2] on the device.
int32_t lm_steps(cude_ctx* c, LmArgs& a, InfoTables& tb) {
    int32_t rc = CUDE_OK;
    const int P = c->P, K = a.K;
    const int64_t N = c->N;
    if ((rc = run_ensemble(c, true, nullptr))) return rc;
    InfoRequest rq;
    rq.want_a = true;
    if ((rc = info_pass(c, rq, tb))) return rc;
    a.A = tb.gn; a.b = tb.ia.b; a.d = tb.ia.d; a.status = tb.ia.status; a.nfail = tb.nfail;
    const hipStream_t s = c->stream;
    hipLaunchKernelGGL(lm_scale_kernel, dim3(1), dim3(kLmThreads), 0, s, a);
    hipLaunchKernelGGL(lm_tables_kernel, dim3(lm_blocks(N), (unsigned)P, (unsigned)K), dim3(kLmThreads), 0, s, a);
    HIP_TRY(hipGetLastError());
    // the Schur sums: one table of weight 1 per damping through the information pass's cross kernel and its partials
    for (int k = 0; k < K; k++) {
        HIP_TRY(cude::launch_info_cross(tb.ia, 1, -1, true, a.tab + (size_t)k * P * N, tb.ia.status, a.part, s));
        HIP_TRY(cude::launch_info_cross_finish(tb.ia, a.part, a.X + (size_t)k * P * P, s));
    }
    hipLaunchKernelGGL(lm_rhs_kernel, dim3((unsigned)P, (unsigned)K), dim3(kLmThreads), 0, s, a);
    const size_t lds = sizeof(double) * ((size_t)P + (a.use_lds ? (size_t)P * P : 0));
    hipLaunchKernelGGL(lm_cholesky_kernel, dim3((unsigned)K), dim3(kLmThreads), lds, s, a);
    hipLaunchKernelGGL(lm_candidates_kernel, dim3(lm_blocks(N), (unsigned)K), dim3(kLmThreads), 0, s, a);
    hipLaunchKernelGGL(lm_pred_kernel, dim3((unsigned)K), dim3(kLmThreads), 0, s, a);
    HIP_TRY(hipGetLastError());
    // the trial losses: one multi-set forward launch, as cude_multistart_forward's
    if ((rc = reserve_sets_forward(c, K, false, c->lm_part))) return rc;
    SetsForward fwd;
    fwd.cond = a.cond_sets; fwd.nn = a.nn_sets; fwd.stride_nn = P; fwd.partials = c->lm_part.p; fwd.n_sets = K;
    if ((rc = forward_sets(c, fwd))) return rc;
    HIP_TRY(cude::launch_reduce_sets(c->lm_part.p, K, c->nblocks, P + 2, P, a.sums, s));
    hipLaunchKernelGGL(lm_losses_kernel, dim3(1), dim3(64), 0, s, a);
    HIP_TRY(hipGetLastError());
    return CUDE_OK;
}
}  // namespace

extern "C" {

int32_t cude_lm_candidates(cude_ctx* c, int32_t n_mu, const double* mu, double* nn_out, double* cond_out, double* pred_out,
                           double* loss_out, double* dnn_out, double* dcond_out) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if ((rc = lm_check_state(c, "cude_lm_candidates"))) return rc;
    if (n_mu < 1 || n_mu > kLmMaxK || !mu) return fail(CUDE_ERR_ARG, "need 1 <= n_mu <= 8 dampings");
    for (int k = 0; k < n_mu; k++)
        if (!(mu[k] > 0.0) || !std::isfinite(mu[k])) return fail(CUDE_ERR_ARG, "dampings must be finite and > 0");
    if (!nn_out && !cond_out && !pred_out && !loss_out && !dnn_out && !dcond_out) return fail(CUDE_ERR_ARG, "no output requested");
    LmArgs a;
    double *nn_bak = nullptr, *cond_bak = nullptr;
    if ((rc = lm_setup(c, n_mu, a, &nn_bak, &cond_bak))) return rc;
    for (int k = 0; k < n_mu; k++) a.mu[k] = mu[k];
    InfoTables tb;
    if ((rc = lm_steps(c, a, tb))) return rc;
    const int P = c->P;
    const int64_t N = c->N;
    std::vector<int32_t> valid((size_t)n_mu);
    HIP_TRY(fetch(c, nn_out, a.nn_sets, (size_t)n_mu * P));
    HIP_TRY(fetch(c, cond_out, a.cond_sets, (size_t)n_mu * N));
    HIP_TRY(fetch(c, pred_out, a.pred, (size_t)n_mu));
    HIP_TRY(fetch(c, loss_out, a.loss, (size_t)n_mu));
    HIP_TRY(fetch(c, dnn_out, a.dth, (size_t)n_mu * P));
    HIP_TRY(fetch(c, dcond_out, a.dcond, (size_t)n_mu * N));
    HIP_TRY(fetch(c, valid.data(), a.valid, (size_t)n_mu));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->last_failed = tb.failed;
    // (an invalid candidate has no step: its sets are NaN for the caller, whatever the trial launch was given)
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int k = 0; k < n_mu; k++) {
        if (valid[(size_t)k]) continue;
        if (nn_out) std::fill(nn_out + (size_t)k * P, nn_out + (size_t)(k + 1) * P, nan);
        if (cond_out) std::fill(cond_out + (size_t)k * N, cond_out + (size_t)(k + 1) * N, nan);
    }
    return CUDE_OK;
}

int32_t cude_train_lm(cude_ctx* c, int32_t max_iters, int32_t n_trials, double mu0, double gtol, double ftol,
                      double* loss_trace, double* mu_trace, int32_t* n_iters_out, int32_t* status_out) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if ((rc = lm_check_state(c, "cude_train_lm"))) return rc;
    if (max_iters < 0) return fail(CUDE_ERR_ARG, "max_iters must be >= 0");
    if (n_trials < 1 || n_trials > kLmMaxK) return fail(CUDE_ERR_ARG, "n_trials must lie in 1 ... 8");
    if (!(mu0 > 0.0) || !std::isfinite(mu0)) return fail(CUDE_ERR_ARG, "mu0 must be finite and > 0");
    if (!(gtol >= 0.0) || !(ftol >= 0.0)) return fail(CUDE_ERR_ARG, "gtol and ftol must be >= 0");
    const int K = n_trials, P = c->P;
    const int64_t N = c->N;
    LmArgs a;
    double *nn_bak = nullptr, *cond_bak = nullptr;
    if ((rc = lm_setup(c, K, a, &nn_bak, &cond_bak))) return rc;
    double mu = std::min(std::max(mu0, kLmMuMin), kLmMuMax);
    double F = 0.0;
    if ((rc = run_ensemble(c, false, nullptr))) return rc;
    if ((rc = finish_loss(c, &F, nullptr))) return rc;
    if (loss_trace) loss_trace[0] = F;
    if (mu_trace) mu_trace[0] = mu;
    int32_t status = std::isfinite(F) ? CUDE_LM_MAX_ITERS : CUDE_LM_FAILED;
    int32_t it = 0;
    const auto restore = [&]() -> int32_t {
        HIP_TRY(hipMemcpyAsync(c->nn.p, nn_bak, (size_t)P * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->cond.p, cond_bak, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        return CUDE_OK;
    };
    while (status == CUDE_LM_MAX_ITERS && it < max_iters) {
        lm_ladder(mu, K, a.mu);
        for (int k = 0; k < K; k++) a.mu[k] = std::min(std::max(a.mu[k], kLmMuMin), kLmMuMax);
        InfoTables tb;
        if ((rc = lm_steps(c, a, tb))) return rc;
        hipLaunchKernelGGL(lm_select_kernel, dim3(1), dim3(1), 0, c->stream, a, F);
        HIP_TRY(hipMemcpyAsync(nn_bak, c->nn.p, (size_t)P * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(cond_bak, c->cond.p, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        hipLaunchKernelGGL(lm_commit_kernel, dim3(lm_blocks(N + P)), dim3(kLmThreads), 0, c->stream, a, c->nn.p, c->cond.p);
        HIP_TRY(hipGetLastError());
        // the selected set is confirmed by the evaluation cude_forward makes, whose value the trace carries
        double rec[5] = {0, 0, 0, 0, 0}, Fn = 0.0;
        HIP_TRY(fetch(c, rec, a.rec, 5));
        if ((rc = run_ensemble(c, false, nullptr))) return rc;
        if ((rc = finish_loss(c, &Fn, nullptr))) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        const int sel = (int)rec[3];
        if (rec[1] > 0.0 || rec[2] > 0.0 || !std::isfinite(rec[0])) {
            if ((rc = restore())) return rc;
            c->last_failed = (int64_t)std::max(rec[1], rec[2]);
            status = CUDE_LM_FAILED;
            break;
        }
        if (rec[0] <= gtol) {
            if ((rc = restore())) return rc;
            status = CUDE_LM_GRAD;
            break;
        }
        it++;
        if (sel >= 0 && std::isfinite(Fn) && Fn < F) {
            const double dec = F - Fn;
            const bool small = dec <= ftol * F;
            F = Fn;
            mu = std::min(std::max(a.mu[sel] / kLmRatio, kLmMuMin), kLmMuMax);
            if (small) status = CUDE_LM_DECREASE;
        } else {
            if ((rc = restore())) return rc;
            mu = kLmRatio * kLmRatio * a.mu[K - 1];
            if (mu > kLmMuMax) { mu = kLmMuMax; status = CUDE_LM_STALLED; }
        }
        if (loss_trace) loss_trace[it] = F;
        if (mu_trace) mu_trace[it] = mu;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (status != CUDE_LM_FAILED) c->last_failed = 0;
    if (n_iters_out) *n_iters_out = it;
    if (status_out) *status_out = status;
    return CUDE_OK;
}

}  // extern "C"
