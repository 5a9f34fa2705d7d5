// The fixed-step tangent-linear sweep of both models: one evaluation of a subject's (SSE, score, information sum) at a value
// of its conditional parameter.  The ONE statement of that arithmetic on the device: the sensitivity kernels (cude_sens.hip)
// call it once per subject, the fused per-subject fits (cude_refine.hip) once per trial point of their iteration.
//
// What differs between the two goes through the sweep's arguments:
//   * the subject's constants are loaded by the caller (*_tan_load), once, also when it calls the sweep many times;
//   * `at_obs` is called once per observation time with the interpolated tangents.  The sensitivity kernels store them;
//     the fits pass TanNoStore, and the compiler drops the tangents nothing else reads (c-peptide states 2 and 3).
// Both networks are the exponential-form ones (no tanh table, no LDS biases).  One lane = one subject; the LDS rows are the
// caller's.
#pragma once
#include "cude_device.h"

namespace cude {

// chk: +0.0, or NaN iff an input of the subject (a parameter, the conditional parameter, its data) is non-finite; sse
// already includes it
struct TanSums {
    double sse, score, info, chk;
};

struct TanNoStore {
    __device__ __forceinline__ void operator()(int, double, double, double = 0.0) const {}
};

// ---------------------------------------------------------------------------------- c-peptide models
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

// what a subject's sweeps share: the linear system, u(t_0) = (c0, y20), its k_1 and the second network constant
struct CpepTanConst {
    double a11, a12, a21, a22, f0, c0, y20, K1a0, K1b0;
    double cst1;                                  // (Net::NC > 1)
    double pchk;                                  // NaN iff a shared parameter / cst1 is non-finite
};

template <class Net>
__device__ __forceinline__ CpepTanConst cpep_tan_load(const CpepArgs& a, int64_t i) {
    const double k0 = a.k0[i], k1 = a.k1[i], k2 = a.k2[i], c0 = a.c0[i];
    CpepTanConst k;
    k.a11 = -(k0 + k2); k.a12 = k1; k.a21 = k2; k.a22 = -k1; k.f0 = k0 * c0;
    k.c0 = c0;
    k.y20 = (k2 / k1) * c0;
    k.K1a0 = fma(k.a11, c0, fma(k.a12, k.y20, k.f0));
    k.K1b0 = fma(k.a21, c0, k.a22 * k.y20);
    k.cst1 = Net::NC > 1 ? a.age[i] : 0.0;
    k.pchk = Net::NC > 1 ? fma(k.cst1, 0.0, Net::param_check(as_const(a.nn))) : Net::param_check(as_const(a.nn));
    return k;
}

// Net: Mlp<NIN, W, D, 1, false, false, HA, OA> or MmProd<RAW>.  NS = 3: + the tangent of the cumulative-secretion quadrature
// state (it enters no residual).  s_q: [5][2][kBlock] stage forcings and their tangents.  at_obs(oi, d u1, d u2, d u3).
//   The production does not depend on the state, so d prod / d cond is a FORCING of the linear tangent system
//   s' = A s + [d q / d cond; 0]: the step's Runge-Kutta algebra runs a second time on (s, dq) with f0 = 0.
template <class Net, int NS, class AtObs>
__device__ __forceinline__ TanSums cpep_tan_sweep(const CpepArgs& a, const CpepTanConst& k, int64_t i, int lane, double cond,
                                                  double* s_q, const AtObs& at_obs) {
    constexpr int NC = Net::NC;
    const int64_t N = a.N;
    cptr_t p = as_const(a.nn);
    cptr_t phi = as_const(a.phi);
    cptr_t obs_w = as_const(a.obs_w);
    ciptr_t seg = as_const(a.seg);
    ciptr_t obs_step = as_const(a.obs_step);
    const int S = a.S, T = a.T;
    const double h = a.h;
    const double a11 = k.a11, a12 = k.a12, a21 = k.a21, a22 = k.a22, f0 = k.f0;

    double cst[NC];
    cst[0] = Net::cond_input(cond);
    if (NC > 1) cst[1] = k.cst1;
    double c[Net::NCST], dc[Net::NCST];
    Net::first_layer_offset(p, cst, c);
    Net::cond_tangent(p, cst[0], dc);

    double y1 = k.c0, y2 = k.y20;
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;                    // d y / d cond: u0 depends on no parameter
    double qprev = 0.0, dqprev = 0.0;                       // q(t_0) = NN(0, .) - NN(0, .) == 0
    double K1a = k.K1a0, K1b = k.K1b0;                      // k_1 of the current step (FSAL)
    double D1a = 0.0, D1b = 0.0;                            // ... and of the tangent system
    int cur_seg = -1;
    double g_lo = 0.0, g_d = 0.0;
    double sse = 0.0, info = 0.0, score = 0.0, base = 0.0, dbase = 0.0;
    // NaN iff an input is non-finite.  (The terms enter as x * 0 + chk, each +0.0 or NaN: the order in which they are
    // chained -- here cst[1] and the parameters first, because they are the subject's, then cond, then the data -- cannot
    // change the result.)
    double chk = fma(cst[0], 0.0, k.pchk);
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
        double s3n = s3;
        if (NS == 3) {
            double d3 = 0.0;
#pragma unroll
            for (int j = 0; j < 6; j++) d3 = fma(Tab::a(6, j), dq[j], d3);
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
            const double res = o1 - a.obs[(int64_t)oi * N + i];
            sse = fma(res, res, sse);
            info = fma(d1, d1, info);
            score = fma(res, d1, score);
            at_obs(oi, d1, d2, d3);
            oi++;
        }
        y1 = Y1; y2 = Y2;
        s1 = S1; s2 = S2; s3 = s3n;
        K1a = K[6][0]; K1b = K[6][1];
        D1a = DK[6][0]; D1b = DK[6][1];
        qprev = q[6];
        dqprev = dq[6];
        n++;
    }
    sse += chk;
    return {sse, score, info, chk};
}

// ---------------------------------------------------------------------------------- suppression model
// u(t_0); u1 of every later time is u10 times a table entry (SuppArgs::rho, obs_rho)
struct SuppTanConst {
    double u10, u20, u30;
    double pchk;                                  // NaN iff a shared parameter / u(t_0) is non-finite
};

template <class Net>
__device__ __forceinline__ SuppTanConst supp_tan_load(const SuppArgs& a, int64_t i) {
    const int64_t N = a.N;
    const int T = a.T;
    SuppTanConst k;
    k.u10 = a.data[((int64_t)0 * T + 0) * N + i];
    k.u20 = a.data[((int64_t)1 * T + 0) * N + i];
    k.u30 = a.data[((int64_t)2 * T + 0) * N + i];
    k.pchk = fma(k.u10 + k.u20 + k.u30, 0.0, Net::param_check(as_const(a.nn)));
    return k;
}

// Net: Mlp<4, W, D, 3, false, false, HA, OA>.  The network reads the state, so the tangent needs the full JVP in x (the
// state's tangent) and in the conditional column (the first-layer offsets).  State 1 depends on no parameter: its tangent is
// exactly 0 and is not carried.  s_K: [7][4][kBlock] stage derivatives of (u2, u3, du2, du3).  at_obs(oi, d u2, d u3).
template <class Net, class AtObs>
__device__ __forceinline__ TanSums supp_tan_sweep(const SuppArgs& a, const SuppTanConst& k, int64_t i, int lane, double cond,
                                                  double* s_K, const AtObs& at_obs) {
    const int64_t N = a.N;
    cptr_t p = as_const(a.nn);
    cptr_t obs_w = as_const(a.obs_w);
    cptr_t rho = as_const(a.rho);
    cptr_t obs_rho = as_const(a.obs_rho);
    ciptr_t obs_step = as_const(a.obs_step);
    const int S = a.S, T = a.T;
    const double h = a.h;
    const double u10 = k.u10;
#define KROW(j, s) s_K[((j) * 4 + (s)) * kBlock + lane]

    const double cst0 = exp(cond);
    const double cst[1] = {cst0};
    double c[Net::NCST], dc[Net::NCST];
    Net::first_layer_offset(p, cst, c);
    Net::cond_tangent(p, cst0, dc);
#pragma unroll
    for (int j = 0; j < 7; j++)
#pragma unroll
        for (int s = 0; s < 4; s++) KROW(j, s) = 0.0;       // (an earlier sweep of the caller may have left NaN in these rows)
    double y[4] = {k.u20, k.u30, 0.0, 0.0};
    const double chk = fma(cst0, 0.0, k.pchk);
    double sse = chk, info = 0.0, score = 0.0;

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
                const double res = u10 * obs_rho[oi] - a.data[((int64_t)0 * T + oi) * N + i];
                sse = fma(res * a.iscale2[0], res, sse);
            }
#pragma unroll
            for (int s = 0; s < 2; s++) {
                const double res = o[s] - a.data[((int64_t)(s + 1) * T + oi) * N + i];
                sse = fma(res * a.iscale2[s + 1], res, sse);
                info = fma(o[2 + s] * a.iscale2[s + 1], o[2 + s], info);
                score = fma(res * a.iscale2[s + 1], o[2 + s], score);
            }
            at_obs(oi, o[2], o[3]);
            oi++;
        }
#pragma unroll
        for (int s = 0; s < 4; s++) { y[s] = u[s]; KROW(0, s) = du[s]; }
        st = 1;
        n++;
    }
#undef KROW
    return {sse, score, info, chk};
}

}  // namespace cude
