// Forward-mode (tangent-linear) ensemble solves for gfx950: every subject's trajectory together with its derivative with
// respect to the subject's own conditional parameter (cude_sensitivity).
//
// Replaces (reference repo paths): the partials every solve of the reference carries under ForwardDiff --
//   sensealg = ForwardDiffSensitivity()                                  src/parameter-estimation.jl:59
//   AutoForwardDiff() through `solve`                                    src/parameter-estimation.jl:165,370
//   the same through the suppression model's ensemble solve             suppression/src/suppression_model.jl:155
// restricted to the per-subject direction d/d(beta_i) resp. d/d(theta_i), which is what standard errors, Wald intervals
// and identifiability flags of a conditional parameter are built from.
//
// One lane = one subject, as cude_cpep.hip / cude_supp_dense.hip; no reduction over subjects except the (sum SSE, failures)
// pair.  The network is evaluated in forward mode (Mlp::eval_jvp / MmProd::eval_jvp, cude_device.h): one sweep gives the
// value and the directional derivative, every weight column is read once for both.
//   * c-peptide models: the production does not depend on the state, so d prod / d beta is a FORCING of the linear tangent
//     system  s' = A s + [d q / d beta; 0]  -- the step's Runge-Kutta algebra simply runs a second time on (s, dq) with
//     f0 = 0.  Five evaluations per step, as the forward kernel.
//   * suppression model: the network reads the state, so the tangent needs the full JVP in x (the state's tangent) and in
//     the theta column (the first-layer offsets).  State 1 depends on no parameter: its tangent is exactly 0 and is not
//     carried; as in the forward kernels its value comes from the closed-form tables (SuppArgs::rho, obs_rho).
//   * adaptive mode: tangent policies (CpepAdTan / SuppAdTan, cude_adaptive.h) over the one-body kernel
//     (cude_adaptive_body.h), instantiated here.
// The networks are the exponential-form ones (no tanh table, no LDS biases): the types the adaptive kernels use.
//
// Failure convention (cude_simulate's): a subject with a non-finite input or a failed adaptive solve gets NaN in all its
// outputs and counts as failed; the other lanes' arithmetic does not depend on it.
//
// The file is compiled in parts (-DCUDE_SENS_PART=k, as cude_adaptive.hip): 0 = c-peptide fixed-step + the dispatchers,
// 1 = c-peptide adaptive, 2 = suppression fixed-step, 3 = suppression adaptive.
#include "cude_adaptive_body.h"
#include "cude_supp.h"

namespace cude {

#ifndef CUDE_SENS_PART
#define CUDE_SENS_PART 0
#endif

hipError_t launch_cpep_sens_adaptive(const NetShape& net, const CpepSensArgs& a, hipStream_t s);
hipError_t launch_supp_sens_fixed(const NetShape& net, const SuppSensArgs& a, hipStream_t s);
hipError_t launch_supp_sens_adaptive(const NetShape& net, const SuppSensArgs& a, hipStream_t s);

// per-subject outputs behind a fixed-step solve (bad: NaN throughout)
template <int NS, class Args>
__device__ __forceinline__ void sens_finish(const Args& a, int64_t i, bool bad, double sse, double info, double score) {
    const double nan = __builtin_nan("");
    if (a.sse != nullptr) a.sse[i] = sse;
    if (a.out.info != nullptr) a.out.info[i] = bad ? nan : info;
    if (a.out.score != nullptr) a.out.score[i] = bad ? nan : score;
    if (bad && a.out.sens != nullptr)
        for (int q = 0; q < NS * a.T; q++) a.out.sens[(int64_t)NS * a.T * i + q] = nan;
}

#if CUDE_SENS_PART == 0
// ---------------------------------------------------------------------------------- c-peptide models, fixed step
// stages 2..7 of one Tsit5 step of  u' = A u + [f0 + q; 0]  from (y1, y2) with K[0] = k_1 given; returns y_{n+1} in (Y1, Y2)
__device__ __forceinline__ void cpep_step_algebra(double a11, double a12, double a21, double a22, double f0, double h,
                                                  double y1, double y2, const double (&q)[7], double (&K)[7][2], double& Y1,
                                                  double& Y2) {
#pragma unroll
    for (int st = 1; st < 7; st++) {
        double t1 = 0.0, t2 = 0.0;
#pragma unroll
        for (int j = 0; j < st; j++) {
            t1 = fma(Tab::a(st, j), K[j][0], t1);
            t2 = fma(Tab::a(st, j), K[j][1], t2);
        }
        Y1 = fma(h, t1, y1);
        Y2 = fma(h, t2, y2);
        K[st][0] = fma(a11, Y1, fma(a12, Y2, f0 + q[st]));
        K[st][1] = fma(a21, Y1, a22 * Y2);
    }
}

// Net: Mlp<NIN, W, D, 1, false, false, HA, OA> or MmProd<RAW>.  NS = 3: + the cumulative-secretion quadrature state.
template <class Net, int NS>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2))) void cpep_sens_kernel(CpepSensArgs a) {
    constexpr int P = Net::P;
    constexpr int NC = Net::NC;
    extern __shared__ double smem[];
    double* s_q = smem;                         // [5][2][kBlock] stage forcings and their tangents
    double* s_red = smem + 10 * kBlock;         // [kRedRows][kBlock]
    const int lane = threadIdx.x;
    const int64_t gid = (int64_t)blockIdx.x * kBlock + lane;
    const bool active = gid < a.N;
    const int64_t i = active ? gid : a.N - 1;
    const int64_t N = a.N;
    cptr_t p = as_const(a.nn);
    cptr_t phi = as_const(a.phi);
    cptr_t obs_w = as_const(a.obs_w);
    ciptr_t seg = as_const(a.seg);
    ciptr_t obs_step = as_const(a.obs_step);
    const int S = a.S, T = a.T;
    const double h = a.h;

    const double k0 = a.k0[i], k1 = a.k1[i], k2 = a.k2[i], c0 = a.c0[i];
    const double a11 = -(k0 + k2), a12 = k1, a21 = k2, a22 = -k1, f0 = k0 * c0;
    double cst[NC];
    cst[0] = Net::cond_input(a.cond[i]);
    if (NC > 1) cst[1] = a.age[i];
    double c[Net::NCST], dc[Net::NCST];
    Net::first_layer_offset(p, cst, c);
    Net::cond_tangent(p, cst[0], dc);

    double y1 = c0, y2 = (k2 / k1) * c0, y3 = 0.0;
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;                    // d y / d cond: u0 depends on no parameter
    double qprev = 0.0, dqprev = 0.0;                       // q(t_0) = NN(0, .) - NN(0, .) == 0
    double K1a = fma(a11, y1, fma(a12, y2, f0)), K1b = fma(a21, y1, a22 * y2);     // k_1 of the current step (FSAL)
    double D1a = 0.0, D1b = 0.0;                            // ... and of the tangent system
    int cur_seg = -1;
    double g_lo = 0.0, g_d = 0.0;
    double sse = 0.0, info = 0.0, score = 0.0, base = 0.0, dbase = 0.0;
    double chk = fma(cst[0], 0.0, Net::param_check(p));     // NaN iff a parameter / beta is non-finite
    if (NC > 1) chk = fma(cst[1], 0.0, chk);
    int oi = 0, n = 0, s = -1;
    // evaluation e = -1 is the baseline NN([0; e^beta]); e = 5n+s is the s-th distinct stage time of step n (cpep_kernel)
#pragma unroll 1
    for (int e = -1; e < 5 * S; e++) {
        double xv = 0.0;
        if (e >= 0) {
            const int sg = seg[e];
            const double ph = phi[e];
            if (sg != cur_seg) {
                cur_seg = sg;
                g_lo = a.dG[(int64_t)sg * N + i];
                g_d = a.dG[(int64_t)(sg + 1) * N + i] - g_lo;
                chk = fma(g_d, 0.0, fma(g_lo, 0.0, chk));
            }
            xv = fma(ph, g_d, g_lo);
        }
        const double x[1] = {xv}, dx[1] = {0.0};
        double dv;
        const double v = Net::template eval_jvp<false>(p, c, x, dc, dx, &dv);
        if (e < 0) { base = v; dbase = dv; s = 0; continue; }
        s_q[(2 * s) * kBlock + lane] = v - base;
        s_q[(2 * s + 1) * kBlock + lane] = dv - dbase;
        if (++s < 5) continue;
        s = 0;
        // ---- step n: the same algebra on (y, q) and on (s, dq)
        double q[7], dq[7];
        q[0] = qprev;
        dq[0] = dqprev;
#pragma unroll
        for (int j = 0; j < 5; j++) {
            q[j + 1] = s_q[(2 * j) * kBlock + lane];
            dq[j + 1] = s_q[(2 * j + 1) * kBlock + lane];
        }
        q[6] = q[5];
        dq[6] = dq[5];
        double K[7][2], DK[7][2];
        K[0][0] = K1a; K[0][1] = K1b;
        DK[0][0] = D1a; DK[0][1] = D1b;
        double Y1 = y1, Y2 = y2, S1 = s1, S2 = s2;
        cpep_step_algebra(a11, a12, a21, a22, f0, h, y1, y2, q, K, Y1, Y2);
        cpep_step_algebra(a11, a12, a21, a22, 0.0, h, s1, s2, dq, DK, S1, S2);
        double y3n = y3, s3n = s3;
        if (NS == 3) {
            double t3 = 0.0, d3 = 0.0;
#pragma unroll
            for (int j = 0; j < 6; j++) {
                t3 = fma(Tab::a(6, j), q[j], t3);
                d3 = fma(Tab::a(6, j), dq[j], d3);
            }
            y3n = fma(h, t3, y3);
            s3n = fma(h, d3, s3);
        }
        while (oi < T && obs_step[oi] == n) {
            double o1 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0;
#pragma unroll
            for (int j = 0; j < 7; j++) {
                const double w = obs_w[oi * 7 + j];
                o1 = fma(w, K[j][0], o1);
                d1 = fma(w, DK[j][0], d1);
                d2 = fma(w, DK[j][1], d2);
                if (NS == 3) d3 = fma(w, dq[j], d3);
            }
            o1 = fma(h, o1, y1);
            d1 = fma(h, d1, s1);
            d2 = fma(h, d2, s2);
            d3 = fma(h, d3, s3);
            const double r = o1 - a.obs[(int64_t)oi * N + i];
            sse = fma(r, r, sse);
            info = fma(d1, d1, info);
            score = fma(r, d1, score);
            if (a.out.sens != nullptr && active) {
                double* tr = a.out.sens + (int64_t)NS * (oi + (int64_t)T * i);
                tr[0] = d1;
                tr[1] = d2;
                if (NS == 3) tr[2] = d3;
            }
            oi++;
        }
        y1 = Y1; y2 = Y2; y3 = y3n;
        s1 = S1; s2 = S2; s3 = s3n;
        K1a = K[6][0]; K1b = K[6][1];
        D1a = DK[6][0]; D1b = DK[6][1];
        qprev = q[6];
        dqprev = dq[6];
        n++;
    }
    sse += chk;
    const bool failed = !(fabs(sse) <= 1.79769313486231570815e308);   // NaN or Inf
    if (active) sens_finish<NS>(a, i, failed, sse, info, score);
    const double v2[2] = {active ? sse : 0.0, (active && failed) ? 1.0 : 0.0};
    block_reduce_store<2>(v2, s_red, a.partials + (int64_t)blockIdx.x * (P + 2) + P, lane);
}

template <class Net>
static hipError_t launch_cpep_fixed(int n_state, const CpepSensArgs& a, hipStream_t s) {
    const int64_t nblocks = (a.N + kBlock - 1) / kBlock;
    const size_t lds = sizeof(double) * (size_t)(10 + kRedRows) * kBlock;
    if (n_state == 2) hipLaunchKernelGGL((cpep_sens_kernel<Net, 2>), dim3((unsigned)nblocks), dim3(kBlock), lds, s, a);
    else hipLaunchKernelGGL((cpep_sens_kernel<Net, 3>), dim3((unsigned)nblocks), dim3(kBlock), lds, s, a);
    return hipGetLastError();
}

template <int NIN, int W, int D>
static hipError_t launch_cpep_fixed_general(const NetShape& net, int n_state, const CpepSensArgs& a, hipStream_t s) {
#define Y(HA, OA) if (net.hact == HA && net.oact == OA) return launch_cpep_fixed<CpepNetG<NIN, W, D, HA, OA>>(n_state, a, s);
    CUDE_GENERAL_ACTS(Y)
#undef Y
    return hipErrorInvalidValue;
}

hipError_t launch_cpep_sens(const NetShape& net, int n_state, const CpepSensArgs& a, hipStream_t s) {
    if (net.generic() || a.partials == nullptr || a.obs == nullptr || a.T < 1 || a.n_sets > 1) return hipErrorInvalidValue;
    if (a.S == 0) return n_state == 2 ? launch_cpep_sens_adaptive(net, a, s) : hipErrorInvalidValue;
    if (n_state != 2 && n_state != 3) return hipErrorInvalidValue;
    if (net.symbolic())
        return a.cond_raw ? launch_cpep_fixed<MmProd<true>>(n_state, a, s) : launch_cpep_fixed<MmProd<false>>(n_state, a, s);
    if (net.general()) {
#define X(NIN, W, D) if (net.nin == NIN && net.width == W && net.depth == D) return launch_cpep_fixed_general<NIN, W, D>(net, n_state, a, s);
        X(2, 4, 2) X(2, 6, 2) X(3, 4, 2)
#undef X
        return hipErrorInvalidValue;
    }
#define X(NIN, W, D) if (net.nin == NIN && net.width == W && net.depth == D) return launch_cpep_fixed<Mlp<NIN, W, D, 1>>(n_state, a, s);
    CUDE_CPEP_AD_SHAPES(X)
#undef X
    return hipErrorInvalidValue;
}

hipError_t launch_supp_sens(const NetShape& net, const SuppSensArgs& a, hipStream_t s) {
    if (net.nin != 4 || net.generic() || a.partials == nullptr || a.T < 1 || a.n_sets > 1 || a.T_data > 0) return hipErrorInvalidValue;
    return a.S == 0 ? launch_supp_sens_adaptive(net, a, s) : launch_supp_sens_fixed(net, a, s);
}

#elif CUDE_SENS_PART == 1
// ---------------------------------------------------------------------------------- c-peptide models, adaptive
template <class Net>
static hipError_t launch_cpep_tan(const CpepSensArgs& a, hipStream_t s) {
    using M = CpepAdTan<Net>;
    const int64_t nblocks = (a.N + kBlock - 1) / kBlock;
    const size_t lds = sizeof(double) * (size_t)(adaptive_rows<M>(false) + a.TG) * kBlock;
    hipLaunchKernelGGL((adaptive_kernel<M, true, false>), dim3((unsigned)nblocks), dim3(kBlock), lds, s, a);
    return hipGetLastError();
}

template <int NIN, int W, int D>
static hipError_t launch_cpep_tan_general(const NetShape& net, const CpepSensArgs& a, hipStream_t s) {
#define Y(HA, OA) if (net.hact == HA && net.oact == OA) return launch_cpep_tan<CpepNetG<NIN, W, D, HA, OA>>(a, s);
    CUDE_GENERAL_ACTS(Y)
#undef Y
    return hipErrorInvalidValue;
}

hipError_t launch_cpep_sens_adaptive(const NetShape& net, const CpepSensArgs& a, hipStream_t s) {
    if (a.TG < 2 || a.TG > kMaxObs) return hipErrorInvalidValue;
    if (net.symbolic()) return a.cond_raw ? launch_cpep_tan<MmProd<true>>(a, s) : launch_cpep_tan<MmProd<false>>(a, s);
    if (net.general()) {
#define X(NIN, W, D) if (net.nin == NIN && net.width == W && net.depth == D) return launch_cpep_tan_general<NIN, W, D>(net, a, s);
        X(2, 4, 2) X(2, 6, 2) X(3, 4, 2)
#undef X
        return hipErrorInvalidValue;
    }
#define X(NIN, W, D) if (net.nin == NIN && net.width == W && net.depth == D) return launch_cpep_tan<Mlp<NIN, W, D, 1>>(a, s);
    CUDE_CPEP_AD_SHAPES(X)
#undef X
    return hipErrorInvalidValue;
}

#elif CUDE_SENS_PART == 2
// ---------------------------------------------------------------------------------- suppression model, fixed step
// supp_dense_kernel's sweep (cude_supp_dense.hip) with the tangents of states 2 and 3 next to them and the residuals formed
template <int W, int D, int HA, int OA>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2))) void supp_sens_kernel(SuppSensArgs a) {
    using Net = Mlp<4, W, D, 3, false, false, HA, OA>;
    constexpr int P = Net::P;
    extern __shared__ double smem[];
    double* s_K = smem;                  // [7][4] stage derivatives of (u2, u3, du2, du3); the reduction's rows afterwards
    const int lane = threadIdx.x;
    const int64_t gid = (int64_t)blockIdx.x * kBlock + lane;
    const bool active = gid < a.N;
    const int64_t i = active ? gid : a.N - 1;
    const int64_t N = a.N;
    cptr_t p = as_const(a.nn);
    cptr_t obs_w = as_const(a.obs_w);
    cptr_t rho = as_const(a.rho);
    cptr_t obs_rho = as_const(a.obs_rho);
    ciptr_t obs_step = as_const(a.obs_step);
    const int S = a.S, T = a.T;
    const double h = a.h;
#define KROW(j, s) s_K[((j) * 4 + (s)) * kBlock + lane]

    const double cst0 = exp(a.cond[i]);
    const double cst[1] = {cst0};
    double c[W], dc[W];
    Net::first_layer_offset(p, cst, c);
    Net::cond_tangent(p, cst0, dc);
#pragma unroll
    for (int j = 0; j < 7; j++)
#pragma unroll
        for (int s = 0; s < 4; s++) KROW(j, s) = 0.0;

    const double u10 = a.data[((int64_t)0 * T + 0) * N + i];     // u1(t_0): every later u1 is this times a table entry
    double y[4] = {a.data[((int64_t)1 * T + 0) * N + i], a.data[((int64_t)2 * T + 0) * N + i], 0.0, 0.0};
    double sse = fma(cst0 + u10 + y[0] + y[1], 0.0, Net::param_check(p));   // NaN iff an input of this subject is non-finite
    double info = 0.0, score = 0.0;

    // evaluation e = 0 is k_1 of step 0; e = 6n+st (st = 1..6) is stage st+1 of step n (st = 6: k_7 = f(y_{n+1}))
    int oi = 0, n = 0, st = 0;
#pragma unroll 1
    for (int e = 0; e <= 6 * S; e++) {
        double u[4];
        const double u1 = u10 * rho[e];
        if (st == 0) {
#pragma unroll
            for (int s = 0; s < 4; s++) u[s] = y[s];
        } else {
            double t[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int j = 0; j < 6; j++) {
                const double aj = TS_A[st][j];
#pragma unroll
                for (int s = 0; s < 4; s++) t[s] = fma(aj, KROW(j, s), t[s]);
            }
#pragma unroll
            for (int s = 0; s < 4; s++) u[s] = fma(h, t[s], y[s]);
        }
        double du[4];
        {
            const double x[3] = {u1, u[0], u[1]}, dx[3] = {0.0, u[2], u[3]};
            double duh;
            const double uh = Net::template eval_jvp<true>(p, c, x, dc, dx, &duh);
            du[0] = fma(0.4, u1, -uh);
            du[1] = fma(-0.3, u[1], uh);
            du[2] = -duh;
            du[3] = fma(-0.3, u[3], duh);
        }
#pragma unroll
        for (int s = 0; s < 4; s++) KROW(st, s) = du[s];
        if (e == 0) { st = 1; continue; }
        if (st < 6) { st++; continue; }
        // ---- end of step n: u = y_{n+1}, KROW(6) = k_7; the observations inside (t_n, t_{n+1}]
        while (oi < T && obs_step[oi] == n) {
            double o[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
            for (int j = 0; j < 7; j++) {
                const double w = obs_w[oi * 7 + j];
#pragma unroll
                for (int s = 0; s < 4; s++) o[s] = fma(w, KROW(j, s), o[s]);
            }
#pragma unroll
            for (int s = 0; s < 4; s++) o[s] = fma(h, o[s], y[s]);
            {
                const double r = u10 * obs_rho[oi] - a.data[((int64_t)0 * T + oi) * N + i];
                sse = fma(r * a.iscale2[0], r, sse);
            }
#pragma unroll
            for (int s = 0; s < 2; s++) {
                const double r = o[s] - a.data[((int64_t)(s + 1) * T + oi) * N + i];
                sse = fma(r * a.iscale2[s + 1], r, sse);
                info = fma(o[2 + s] * a.iscale2[s + 1], o[2 + s], info);
                score = fma(r * a.iscale2[s + 1], o[2 + s], score);
            }
            if (a.out.sens != nullptr && active) {
                double* tr = a.out.sens + (int64_t)3 * (oi + (int64_t)T * i);
                tr[0] = 0.0;
                tr[1] = o[2];
                tr[2] = o[3];
            }
            oi++;
        }
#pragma unroll
        for (int s = 0; s < 4; s++) { y[s] = u[s]; KROW(0, s) = du[s]; }
        st = 1;
        n++;
    }
#undef KROW
    const bool failed = !(fabs(sse) <= 1.79769313486231570815e308);
    if (active) sens_finish<3>(a, i, failed, sse, info, score);
    const double v2[2] = {active ? sse : 0.0, (active && failed) ? 1.0 : 0.0};
    block_reduce_store<2>(v2, smem, a.partials + (int64_t)blockIdx.x * (P + 2) + P, lane);
}

template <int W, int D, int HA = kActHiddenTanh, int OA = kActOutSoftplus>
static hipError_t launch_supp_fixed(const SuppSensArgs& a, hipStream_t s) {
    const int64_t nblocks = (a.N + kBlock - 1) / kBlock;
    hipLaunchKernelGGL((supp_sens_kernel<W, D, HA, OA>), dim3((unsigned)nblocks), dim3(kBlock),
                       sizeof(double) * (size_t)(7 * 4) * kBlock, s, a);
    return hipGetLastError();
}

template <int W, int D>
static hipError_t launch_supp_fixed_general(const NetShape& net, const SuppSensArgs& a, hipStream_t s) {
#define Y(HA, OA) if (net.hact == HA && net.oact == OA) return launch_supp_fixed<W, D, HA, OA>(a, s);
    CUDE_GENERAL_ACTS(Y)
#undef Y
    return hipErrorInvalidValue;
}

hipError_t launch_supp_sens_fixed(const NetShape& net, const SuppSensArgs& a, hipStream_t s) {
    if (a.rho == nullptr || a.obs_rho == nullptr || a.S < 1) return hipErrorInvalidValue;
    if (net.general()) {
#define X(W, D) if (net.width == W && net.depth == D) return launch_supp_fixed_general<W, D>(net, a, s);
        CUDE_SUPP_GENERAL_SHAPES(X)
#undef X
        return hipErrorInvalidValue;
    }
#define X(W, D) if (net.width == W && net.depth == D) return launch_supp_fixed<W, D>(a, s);
    CUDE_SUPP_SHAPES(X)
#undef X
    return hipErrorInvalidValue;
}

#else
// ---------------------------------------------------------------------------------- suppression model, adaptive
template <class M>
static hipError_t launch_supp_tan(const SuppSensArgs& a, hipStream_t s) {
    const int64_t nblocks = (a.N + kBlock - 1) / kBlock;
    const size_t lds = sizeof(double) * (size_t)adaptive_rows<M>(false) * kBlock;
    hipLaunchKernelGGL((adaptive_kernel<M, false, false>), dim3((unsigned)nblocks), dim3(kBlock), lds, s, a);
    return hipGetLastError();
}

template <int W, int D>
static hipError_t launch_supp_tan_general(const NetShape& net, const SuppSensArgs& a, hipStream_t s) {
#define Y(HA, OA) if (net.hact == HA && net.oact == OA) return launch_supp_tan<SuppAdTan<W, D, HA, OA>>(a, s);
    CUDE_GENERAL_ACTS(Y)
#undef Y
    return hipErrorInvalidValue;
}

hipError_t launch_supp_sens_adaptive(const NetShape& net, const SuppSensArgs& a, hipStream_t s) {
    if (net.general()) {
#define X(W, D) if (net.width == W && net.depth == D) return launch_supp_tan_general<W, D>(net, a, s);
        CUDE_SUPP_GENERAL_SHAPES(X)
#undef X
        return hipErrorInvalidValue;
    }
#define X(W, D) if (net.width == W && net.depth == D) return launch_supp_tan<SuppAdTan<W, D>>(a, s);
    CUDE_SUPP_SHAPES(X)
#undef X
    return hipErrorInvalidValue;
}
#endif

}  // namespace cude
