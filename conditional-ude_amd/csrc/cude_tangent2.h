// The fixed-step ORDER-2 forward-mode sweep of both models: one evaluation of a subject's (SSE, score, information sum,
// second-order sum) at a value of its conditional parameter, with u, s = d u / d cond and r = d^2 u / d cond^2 carried
// together.  The curvature kernels (cude_curv.hip) call it once per subject.
//
// It is cude_tangent.h's sweep carried one Taylor coefficient further, and it is stated here and not as a template
// parameter of those functions: with the order as a parameter the order-1 instantiations (cude_sensitivity,
// cude_refine_conditional) compiled to differently scheduled code, and those kernels are held to the bits they return.
// What the two files share is used from there: cpep_step_algebra, the subject's constants (*_tan_load), TanSums.
//
// The result is the exact second derivative of the DISCRETE map -- every stage, the FSAL carry and the dense-output weights
// obs_w -- not a discretisation of a second-order sensitivity equation.  The primal and first-order operations are those of
// cude_tangent.h in the same order.  One lane = one subject; the LDS rows are the caller's.
#pragma once
#include "cude_tangent.h"

namespace cude {

// curv2 = sum w^2 (yhat - y) d^2 yhat / d cond^2: the curvature (1/2) d^2 SSE_i / d cond_i^2 is info + curv2
struct TanSums2 : TanSums {
    double curv2;
};

// ---------------------------------------------------------------------------------- c-peptide models
// Net, NS: as cpep_tan_sweep.  The production does not read the state, so d^2 q / d cond^2 is a forcing exactly as
// d q / d cond is: the step's Runge-Kutta algebra runs a third time on (r, d2q) with f0 = 0.  s_q: [5][3][kBlock] stage
// forcings with their first and second derivatives.  at_obs(oi, d^2 u1, d^2 u2, d^2 u3).
template <class Net, int NS, class AtObs>
__device__ __forceinline__ TanSums2 cpep_tan2_sweep(const CpepArgs& a, const CpepTanConst& k, int64_t i, int lane, double cond,
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
    double c[Net::NCST], dc[Net::NCST], d2c[Net::NCST];
    Net::first_layer_offset(p, cst, c);
    Net::cond_tangent(p, cst[0], dc);
    Net::cond_tangent2(p, cst[0], d2c);

    double y1 = k.c0, y2 = k.y20;
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;                    // d y / d cond: u0 depends on no parameter
    double r1 = 0.0, r2 = 0.0, r3 = 0.0;                    // d^2 y / d cond^2
    double qprev = 0.0, dqprev = 0.0, d2qprev = 0.0;        // q(t_0) = NN(0, .) - NN(0, .) == 0
    double K1a = k.K1a0, K1b = k.K1b0;                      // k_1 of the current step (FSAL)
    double D1a = 0.0, D1b = 0.0, E1a = 0.0, E1b = 0.0;      // ... and of the two tangent systems
    int cur_seg = -1;
    double g_lo = 0.0, g_d = 0.0;
    double sse = 0.0, info = 0.0, score = 0.0, curv2 = 0.0, base = 0.0, dbase = 0.0, d2base = 0.0;
    double chk = fma(cst[0], 0.0, k.pchk);                  // NaN iff an input is non-finite (cpep_tan_sweep)
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
        double dv, d2v;
        const double v = Net::template eval_jet2<false>(p, c, x, dc, dx, d2c, dx, &dv, &d2v);
        if (e < 0) { base = v; dbase = dv; d2base = d2v; s = 0; continue; }
        s_q[(3 * s) * kBlock + lane] = v - base;
        s_q[(3 * s + 1) * kBlock + lane] = dv - dbase;
        s_q[(3 * s + 2) * kBlock + lane] = d2v - d2base;
        if (++s < 5) continue;
        s = 0;
        // ---- step n: the same algebra on (y, q), on (s, dq) and on (r, d2q)
        double q[7], dq[7], d2q[7];
        q[0] = qprev;
        dq[0] = dqprev;
        d2q[0] = d2qprev;
#pragma unroll
        for (int j = 0; j < 5; j++) {
            q[j + 1] = s_q[(3 * j) * kBlock + lane];
            dq[j + 1] = s_q[(3 * j + 1) * kBlock + lane];
            d2q[j + 1] = s_q[(3 * j + 2) * kBlock + lane];
        }
        q[6] = q[5];
        dq[6] = dq[5];
        d2q[6] = d2q[5];
        double K[7][2], DK[7][2], EK[7][2];
        K[0][0] = K1a; K[0][1] = K1b;
        DK[0][0] = D1a; DK[0][1] = D1b;
        EK[0][0] = E1a; EK[0][1] = E1b;
        double Y1 = y1, Y2 = y2, S1 = s1, S2 = s2, R1 = r1, R2 = r2;
        cpep_step_algebra(a11, a12, a21, a22, f0, h, y1, y2, q, K, Y1, Y2);
        cpep_step_algebra(a11, a12, a21, a22, 0.0, h, s1, s2, dq, DK, S1, S2);
        cpep_step_algebra(a11, a12, a21, a22, 0.0, h, r1, r2, d2q, EK, R1, R2);
        double s3n = s3, r3n = r3;
        if (NS == 3) {
            double d3 = 0.0, e3 = 0.0;
#pragma unroll
            for (int j = 0; j < 6; j++) {
                d3 = fma(Tab::a(6, j), dq[j], d3);
                e3 = fma(Tab::a(6, j), d2q[j], e3);
            }
            s3n = fma(h, d3, s3);
            r3n = fma(h, e3, r3);
        }
        while (oi < T && obs_step[oi] == n) {
            double o1 = 0.0, d1 = 0.0, e1 = 0.0, e2 = 0.0, e3 = 0.0;
#pragma unroll
            for (int j = 0; j < 7; j++) {
                const double w = obs_w[oi * 7 + j];
                o1 = fma(w, K[j][0], o1);
                d1 = fma(w, DK[j][0], d1);
                e1 = fma(w, EK[j][0], e1);
                e2 = fma(w, EK[j][1], e2);
                if (NS == 3) e3 = fma(w, d2q[j], e3);
            }
            o1 = fma(h, o1, y1);
            d1 = fma(h, d1, s1);
            e1 = fma(h, e1, r1);
            e2 = fma(h, e2, r2);
            e3 = fma(h, e3, r3);
            const double res = o1 - a.obs[(int64_t)oi * N + i];
            sse = fma(res, res, sse);
            info = fma(d1, d1, info);
            score = fma(res, d1, score);
            curv2 = fma(res, e1, curv2);
            at_obs(oi, e1, e2, e3);
            oi++;
        }
        y1 = Y1; y2 = Y2;
        s1 = S1; s2 = S2; s3 = s3n;
        r1 = R1; r2 = R2; r3 = r3n;
        K1a = K[6][0]; K1b = K[6][1];
        D1a = DK[6][0]; D1b = DK[6][1];
        E1a = EK[6][0]; E1b = EK[6][1];
        qprev = q[6];
        dqprev = dq[6];
        d2qprev = d2q[6];
        n++;
    }
    sse += chk;
    return {{sse, score, info, chk}, curv2};
}

// ---------------------------------------------------------------------------------- suppression model
// Net: as supp_tan_sweep.  States 2 and 3 carry (u, s, r); state 1 depends on no parameter and carries nothing.  The network
// gets dx = (0, s2, s3) and d2x = (0, r2, r3) at every stage.  s_K: [7][6][kBlock] stage derivatives of
// (u2, u3, s2, s3, r2, r3).  at_obs(oi, d^2 u2, d^2 u3).
template <class Net, class AtObs>
__device__ __forceinline__ TanSums2 supp_tan2_sweep(const SuppArgs& a, const SuppTanConst& k, int64_t i, int lane, double cond,
                                                    double* s_K, const AtObs& at_obs) {
    constexpr int NQ = 6;
    const int64_t N = a.N;
    cptr_t p = as_const(a.nn);
    cptr_t obs_w = as_const(a.obs_w);
    cptr_t rho = as_const(a.rho);
    cptr_t obs_rho = as_const(a.obs_rho);
    ciptr_t obs_step = as_const(a.obs_step);
    const int S = a.S, T = a.T;
    const double h = a.h;
    const double u10 = k.u10;
#define KROW(j, s) s_K[((j) * NQ + (s)) * kBlock + lane]

    const double cst0 = exp(cond);
    const double cst[1] = {cst0};
    double c[Net::NCST], dc[Net::NCST], d2c[Net::NCST];
    Net::first_layer_offset(p, cst, c);
    Net::cond_tangent(p, cst0, dc);
    Net::cond_tangent2(p, cst0, d2c);
#pragma unroll
    for (int j = 0; j < 7; j++)
#pragma unroll
        for (int s = 0; s < NQ; s++) KROW(j, s) = 0.0;
    double y[NQ] = {k.u20, k.u30, 0.0, 0.0, 0.0, 0.0};
    const double chk = fma(cst0, 0.0, k.pchk);
    double sse = chk, info = 0.0, score = 0.0, curv2 = 0.0;

    // evaluation e = 0 is k_1 of step 0; e = 6n+st (st = 1..6) is stage st+1 of step n (st = 6: k_7 = f(y_{n+1}))
    int oi = 0, n = 0, st = 0;
#pragma unroll 1
    for (int e = 0; e <= 6 * S; e++) {
        double u[NQ];
        const double u1 = u10 * rho[e];
        if (st == 0) {
#pragma unroll
            for (int s = 0; s < NQ; s++) u[s] = y[s];
        } else {
            double t[NQ] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int j = 0; j < 6; j++) {
                const double aj = TS_A[st][j];
#pragma unroll
                for (int s = 0; s < NQ; s++) t[s] = fma(aj, KROW(j, s), t[s]);
            }
#pragma unroll
            for (int s = 0; s < NQ; s++) u[s] = fma(h, t[s], y[s]);
        }
        double du[NQ];
        {
            const double x[3] = {u1, u[0], u[1]}, dx[3] = {0.0, u[2], u[3]}, d2x[3] = {0.0, u[4], u[5]};
            double duh, d2uh;
            const double uh = Net::template eval_jet2<true>(p, c, x, dc, dx, d2c, d2x, &duh, &d2uh);
            du[0] = fma(0.4, u1, -uh);
            du[1] = fma(-0.3, u[1], uh);
            du[2] = -duh;
            du[3] = fma(-0.3, u[3], duh);
            du[4] = -d2uh;
            du[5] = fma(-0.3, u[5], d2uh);
        }
#pragma unroll
        for (int s = 0; s < NQ; s++) KROW(st, s) = du[s];
        if (e == 0) { st = 1; continue; }
        if (st < 6) { st++; continue; }
        // ---- end of step n: u = y_{n+1}, KROW(6) = k_7; the observations inside (t_n, t_{n+1}]
        while (oi < T && obs_step[oi] == n) {
            double o[NQ] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
            for (int j = 0; j < 7; j++) {
                const double w = obs_w[oi * 7 + j];
#pragma unroll
                for (int s = 0; s < NQ; s++) o[s] = fma(w, KROW(j, s), o[s]);
            }
#pragma unroll
            for (int s = 0; s < NQ; s++) o[s] = fma(h, o[s], y[s]);
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
                curv2 = fma(res * a.iscale2[s + 1], o[4 + s], curv2);
            }
            at_obs(oi, o[4], o[5]);
            oi++;
        }
#pragma unroll
        for (int s = 0; s < NQ; s++) { y[s] = u[s]; KROW(0, s) = du[s]; }
        st = 1;
        n++;
    }
#undef KROW
    return {{sse, score, info, chk}, curv2};
}

}  // namespace cude
