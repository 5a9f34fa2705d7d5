// Adaptive Tsit5 on the device: tableau rows, tolerances and the model policies shared by the two integrators
// (cude_adaptive.hip: one network body walked through every phase; cude_adaptive_unrolled.hip: the stages of a step
// unrolled, for the constant-Jacobian models on short sampling grids).
#pragma once
#include "cude_device.h"
#include "cude_kernels.h"

namespace cude {

__device__ __constant__ const double TS_C[7] = {0.0, 0.161, 0.327, 0.9, 0.9800255409045097, 1.0, 1.0};
__device__ __constant__ const double TS_BT[7] = {-0.00178001105222577714, -0.0008164344596567469, 0.007880878010261995,
                                                 -0.1447110071732629, 0.5823571654525552, -0.45808210592918697,
                                                 0.015151515151515152};
__device__ __constant__ const double TS_R[7][4] = {{1.0, -2.763706197274826, 2.9132554618219126, -1.0530884977290216},
                                                   {0.0, 0.13169999999999998, -0.2234, 0.1017},
                                                   {0.0, 3.9302962368947516, -5.941033872131505, 2.490627285651253},
                                                   {0.0, -12.411077166933676, 30.33818863028232, -16.548102889244902},
                                                   {0.0, 37.50931341651104, -88.1789048947664, 47.37952196281928},
                                                   {0.0, -27.896526289197286, 65.09189467479366, -34.87065786149661},
                                                   {0.0, 1.5, -4.0, 2.5}};

constexpr int kAdaptiveMaxSteps = 100000;     // OrdinaryDiffEq's default maxiters
#ifndef CUDE_ADAPT_2W_NACC
#define CUDE_ADAPT_2W_NACC 64
#endif

// ---------------------------------------------------------------------------------- model policies
// c-peptide cUDE / symbolic model: f(t, u) = A u + [k0 c0 + q(t); 0],  q(t) = P(dG(t)) - P(0)
// accumulators pinned behind their updates in every network evaluation of the replay loop (Mlp::eval_grad, PIN)
#ifndef CUDE_ADAPTIVE_PIN
#define CUDE_ADAPTIVE_PIN 1
#endif
constexpr bool kAdaptivePin = CUDE_ADAPTIVE_PIN != 0;

template <class Net>
struct CpepAd {
    static constexpr int NS = 2;
    static constexpr int P = Net::P;
    using Args = CpepArgs;
    double a11, a12, a21, a22, f0, base;
    double c[Net::NCST];
    double cst0;
    const double* s_G;             // [TG][kBlock] glucose increments at the knots (LDS)
    cptr_t tp;
    int TG, lane;
    cptr_t p;
    static __device__ __forceinline__ int lds_rows(const Args& a) { return a.TG; }
    __device__ __forceinline__ double init(const Args& a, double* s_extra, int lane_, int64_t i, int64_t set, double (&y)[NS]) {
        constexpr int NC = Net::NC;
        lane = lane_;
        p = as_const(a.nn + set * a.set_stride_nn);
        tp = as_const(a.tp);
        TG = a.TG;
        const double k0 = a.k0[i], k1 = a.k1[i], k2 = a.k2[i], c0 = a.c0[i];
        a11 = -(k0 + k2); a12 = k1; a21 = k2; a22 = -k1; f0 = k0 * c0;
        double cst[NC];
        cst[0] = Net::cond_input(a.cond[set * a.set_stride_cond + i]);
        if (NC > 1) cst[1] = a.age[i];
        cst0 = cst[0];
        Net::first_layer_offset(p, cst, c);
        double* g = s_extra;
        double chk = fma(cst[0], 0.0, Net::param_check(p));
        if (NC > 1) chk = fma(cst[1], 0.0, chk);
        for (int m = 0; m < TG; m++) {
            const double v = a.dG[(int64_t)m * a.N + i];
            g[m * kBlock + lane] = v;
            chk = fma(v, 0.0, chk);
        }
        s_G = g;
        y[0] = c0;
        y[1] = (k2 / k1) * c0;
        base = 0.0;
        return chk;                               // NaN iff an input of this subject is non-finite
    }
    // network input at time t: glucose(t) - glucose(t_0), linear between the knots (DataInterpolations.LinearInterpolation)
    __device__ __forceinline__ double forcing_input(double t) const {
        int j = 0;
        double tlo = tp[0], thi = tp[1];
        for (int m = 1; m < TG - 1; m++) {
            const double tm = tp[m];
            if (tm <= t) { j = m; tlo = tm; thi = tp[m + 1]; }
        }
        const double glo = s_G[j * kBlock + lane], ghi = s_G[(j + 1) * kBlock + lane];
        return fma(t - tlo, (ghi - glo) / (thi - tlo), glo);
    }
    // production P(x) (the only network call site of the kernel goes through here)
    __device__ __forceinline__ double production(double x) const {
        const double xx[1] = {x};
        return Net::eval(p, c, xx);
    }
    __device__ __forceinline__ void finish_rhs(double prod, const double (&u)[NS], double (&du)[NS]) const {
        du[0] = fma(a11, u[0], fma(a12, u[1], f0 + (prod - base)));
        du[1] = fma(a21, u[0], a22 * u[1]);
    }
    __device__ __forceinline__ double residual2(const Args& a, int oi, int64_t i, const double (&o)[NS], bool active) const {
        if (a.traj != nullptr && active) {
            double* tr = a.traj + (int64_t)NS * (oi + (int64_t)a.T * i);
            tr[0] = o[0];
            tr[1] = o[1];
        }
        if (a.obs == nullptr) return 0.0;
        const double r = o[0] - a.obs[(int64_t)oi * a.N + i];
        return r * r;
    }
    // ---- gradient
    static constexpr int A0 = 0;                   // first state that has an adjoint
    static constexpr bool NEED_Y = false;          // J_f = A: the stage inputs are not linearisation points
    using NetT = Net;
    static constexpr int NCST = Net::NC;
    // d residual2 / d o
    __device__ __forceinline__ void residual_bar(const Args& a, int oi, int64_t i, const double (&o)[NS], double (&ob)[NS]) const {
        ob[0] = 2.0 * (o[0] - a.obs[(int64_t)oi * a.N + i]);
        ob[1] = 0.0;
    }
    // ... replaced by the unit seed of set `set` (kernels compiled with ROWS, Args::unit_seed > 0)
    __device__ __forceinline__ void unit_bar(const Args& a, int oi, int64_t set, double (&ob)[NS]) const {
        ob[0] = unit_seed_cpep(a, set, oi);
        ob[1] = 0.0;
    }
    // acc += wgt * d production(te) / d params  (the baseline term is collected by the caller)
    template <class A>
    __device__ __forceinline__ void vjp_net(double te, double wgt, A& acc) const {
        const double xx[1] = {forcing_input(te)};
        double dx[1] = {0.0};
        Net::template eval_grad<false, A, kAdaptivePin>(p, c, xx, wgt, acc, dx);
    }
    __device__ __forceinline__ void vjp_linear(const double (&kb)[NS], double (&ub)[NS]) const {
        ub[0] += fma(a11, kb[0], a21 * kb[1]);
        ub[1] += fma(a12, kb[0], a22 * kb[1]);
    }
    template <class A>
    __device__ __forceinline__ void finish_grad(const Args& a, int64_t i, int64_t set, A& acc, double wsum, double carry,
                                                double (&cst)[NCST]) const {
        double dx[1] = {0.0};
        // one call site for the two closing evaluations: k_1 of the first step (time t_0, weight carry), then the
        // baseline term  - sum(kb) * d NN([0; e^beta]) / d params
#pragma unroll 1
        for (int r = 0; r < 2; r++) {
            const double xx[1] = {r == 0 ? forcing_input(a.t_begin) : 0.0};
            Net::template eval_grad<false, A, kAdaptivePin>(p, c, xx, r == 0 ? carry : -wsum, acc, dx);
        }
        cst[0] = Net::cond_input(a.cond[set * a.set_stride_cond + i]);
        if (NCST > 1) cst[NCST - 1] = a.age[i];
    }
};

// suppression cUDE: f(u) = [-0.4 u1, 0.4 u1 - NN(u, e^theta), NN(u, e^theta) - 0.3 u3]
template <int W, int D, int HA = kActHiddenTanh, int OA = kActOutSoftplus>
struct SuppAd {
    static constexpr int NS = 3;
    using Net = Mlp<4, W, D, 3, false, false, HA, OA>;
    static constexpr int P = Net::P;
    using Args = SuppArgs;
    double c[W];
    cptr_t p;
    static __device__ __forceinline__ int lds_rows(const Args&) { return 0; }
    __device__ __forceinline__ double init(const Args& a, double*, int, int64_t i, int64_t set, double (&y)[NS]) {
        p = as_const(a.nn + set * a.set_stride_nn);
        double cst[1] = {exp(a.cond[set * a.set_stride_cond + i])};
        Net::first_layer_offset(p, cst, c);
        double chk = fma(cst[0], 0.0, Net::param_check(p));
#pragma unroll
        for (int s = 0; s < 3; s++) {
            y[s] = a.data[((int64_t)s * a.T + 0) * a.N + i];
            chk = fma(y[s], 0.0, chk);
        }
        return chk;
    }
    __device__ __forceinline__ double residual2(const Args& a, int oi, int64_t i, const double (&o)[NS], bool active) const {
        double s2 = 0.0;
#pragma unroll
        for (int s = 0; s < 3; s++) {
            if (a.traj != nullptr && active) a.traj[s + 3 * (oi + (int64_t)a.T * i)] = o[s];
            const double r = o[s] - a.data[((int64_t)s * a.T + oi) * a.N + i];
            s2 = fma(r * a.iscale2[s], r, s2);
        }
        return s2;
    }
    // ---- gradient
    // State 1 (du1 = -0.4 u1, suppression_model.jl:91) depends on no parameter and on no other state: nothing that
    // reaches d/d(network) or d/d(theta) passes through its adjoint (the VJP weight is kb[2] - kb[1]).  The forward
    // sweep integrates it like the others -- the step-size controller's error norm weighs it -- and the tape keeps it
    // (it is a network input); the reverse sweep carries adjoints for states 2 and 3 only.
    static constexpr int A0 = 1;
    static constexpr bool NEED_Y = true;
    using NetT = Net;
    static constexpr int NCST = 1;
    __device__ __forceinline__ void residual_bar(const Args& a, int oi, int64_t i, const double (&o)[NS], double (&ob)[NS]) const {
        ob[0] = 0.0;
#pragma unroll
        for (int s = 1; s < 3; s++) ob[s] = 2.0 * a.iscale2[s] * (o[s] - a.data[((int64_t)s * a.T + oi) * a.N + i]);
    }
    __device__ __forceinline__ void unit_bar(const Args& a, int oi, int64_t set, double (&ob)[NS]) const {
        ob[0] = 0.0;
#pragma unroll
        for (int s = 1; s < 3; s++) ob[s] = unit_seed_supp(a, set, oi, s);
    }
    template <class A>
    __device__ __forceinline__ void vjp(double, const double (&u)[NS], const double (&kb)[NS], double (&ub)[NS], A& acc,
                                        double&) const {
        const double wgt = kb[2] - kb[1];
        double dx[3] = {0.0, 0.0, 0.0};
        Net::template eval_grad<true, A, kAdaptivePin, 1>(p, c, u, wgt, acc, dx);
        ub[1] += dx[1];
        ub[2] += fma(-0.3, kb[2], dx[2]);
    }
    template <class A>
    __device__ __forceinline__ void finish_grad(const Args& a, int64_t i, int64_t set, A&, double, double,
                                                double (&cst)[NCST]) const {
        cst[0] = exp(a.cond[set * a.set_stride_cond + i]);
    }

};

// the same model in an outputs-only launch (dense output, SuppArgs::T_data > 0): u0 from the data's first column, the
// states written at the output times, no residual (forward only); NaN throughout for a subject with a non-finite input
template <int W, int D, int HA = kActHiddenTanh, int OA = kActOutSoftplus>
struct SuppAdOut : SuppAd<W, D, HA, OA> {
    using Base = SuppAd<W, D, HA, OA>;
    using typename Base::Net;
    using typename Base::Args;
    using Base::NS;
    bool bad;
    __device__ __forceinline__ double init(const Args& a, double*, int, int64_t i, int64_t set, double (&y)[NS]) {
        this->p = as_const(a.nn + set * a.set_stride_nn);
        double cst[1] = {exp(a.cond[set * a.set_stride_cond + i])};
        Net::first_layer_offset(this->p, cst, this->c);
        double chk = fma(cst[0], 0.0, Net::param_check(this->p));
#pragma unroll
        for (int s = 0; s < 3; s++) {
            y[s] = a.data[((int64_t)s * a.T_data + 0) * a.N + i];
            chk = fma(y[s], 0.0, chk);
        }
        bad = !(chk == 0.0);
        return chk;
    }
    __device__ __forceinline__ double residual2(const Args& a, int oi, int64_t i, const double (&o)[NS], bool active) const {
        if (active) {
            double* tr = a.traj + oi * a.traj_st + i * a.traj_sn;
#pragma unroll
            for (int s = 0; s < 3; s++) tr[s * a.traj_ss] = bad ? __builtin_nan("") : o[s];
        }
        return 0.0;
    }
};

// ---------------------------------------------------------------------------------- tangent policies (cude_sensitivity)
// The same solves carrying d u / d(conditional) next to u: the state vector of the one-body kernel is [u; du], the
// right-hand side of the second half is the tangent-linear one (Net::eval_jvp), and the step-size control reads the first
// NERR states only -- so the accepted steps are those of the plain solve (cude_forward) and the tangent is the derivative
// of the accepted-step map, the convention of the adaptive adjoint.  (OrdinaryDiffEq's norm under ForwardDiff duals also
// weighs the partials; that variant is not built: INTEGRATION.md.)  The primal operations are those of CpepAd / SuppAd in
// the same order.  A policy with a member NERR is a tangent policy to the kernel:
//   rhs(st, te, Y, du)               the whole right-hand side (st: the kernel's phase, -2 = k_1 of the first step)
//   record(a, slot, n, t, dt, y)     accepted step n, written in the layout of the gradient's tape (cude_adaptive_steps)
//   finish(a, i, active, bad)        per-subject outputs behind the solve
template <class M, class = void>
struct AdTangent {
    static constexpr bool value = false;
    static constexpr int nerr = M::NS;
};
template <class M>
struct AdTangent<M, decltype((void)M::NERR)> {
    static constexpr bool value = true;
    static constexpr int nerr = M::NERR;
};

template <class Net>
struct CpepAdTan : CpepAd<Net> {
    using Base = CpepAd<Net>;
    static constexpr int NS = 4, NERR = 2;          // [u1, u2, du1, du2]
    using Args = CpepSensArgs;
    double dc[Net::NCST];
    double dbase, prod_last, dprod_last, info, score;
    __device__ __forceinline__ double init(const Args& a, double* s_extra, int lane_, int64_t i, int64_t set, double (&y)[NS]) {
        double y2[2];
        const double chk = Base::init(a, s_extra, lane_, i, set, y2);
        y[0] = y2[0]; y[1] = y2[1]; y[2] = 0.0; y[3] = 0.0;
        Net::cond_tangent(this->p, this->cst0, dc);
        dbase = prod_last = dprod_last = info = score = 0.0;
        return chk;
    }
    __device__ __forceinline__ void rhs(int st, double te, const double (&Y)[NS], double (&du)[NS]) {
        // the forcing depends on time only and c_6 = c_7 = 1: stage 7 (st == 6, wave-uniform) reuses stage 6's value;
        // st == -2: the baseline NN([0; e^beta]) first (one call site for both)
        if (st != 6) {
            const int nr = st == -2 ? 2 : 1;
#pragma unroll 1
            for (int r = 0; r < nr; r++) {
                const bool is_base = st == -2 && r == 0;
                const double xx[1] = {is_base ? 0.0 : this->forcing_input(te)}, dx[1] = {0.0};
                double dv;
                const double v = Net::template eval_jvp<false>(this->p, this->c, xx, dc, dx, &dv);
                if (is_base) { this->base = v; dbase = dv; }
                else { prod_last = v; dprod_last = dv; }
            }
        }
        du[0] = fma(this->a11, Y[0], fma(this->a12, Y[1], this->f0 + (prod_last - this->base)));
        du[1] = fma(this->a21, Y[0], this->a22 * Y[1]);
        du[2] = fma(this->a11, Y[2], fma(this->a12, Y[3], dprod_last - dbase));
        du[3] = fma(this->a21, Y[2], this->a22 * Y[3]);
    }
    __device__ __forceinline__ double residual2(const Args& a, int oi, int64_t i, const double (&o)[NS], bool active) {
        if (a.out.sens != nullptr && active) {
            double* tr = a.out.sens + (int64_t)2 * (oi + (int64_t)a.T * i);
            tr[0] = o[2];
            tr[1] = o[3];
        }
        const double r = o[0] - a.obs[(int64_t)oi * a.N + i];
        info = fma(o[2], o[2], info);
        score = fma(r, o[2], score);
        return r * r;
    }
    __device__ __forceinline__ void record(const Args& a, int64_t slot, int n, double, double dt, const double (&)[NS]) const {
        if (a.tape != nullptr && n < a.tape_cap) a.tape[(int64_t)n * a.N + slot] = dt;
    }
    __device__ __forceinline__ void finish(const Args& a, int64_t i, bool active, bool bad) const {
        if (!active) return;
        const double nan = __builtin_nan("");
        if (a.out.info != nullptr) a.out.info[i] = bad ? nan : info;
        if (a.out.score != nullptr) a.out.score[i] = bad ? nan : score;
        if (bad && a.out.sens != nullptr)
            for (int q = 0; q < 2 * a.T; q++) a.out.sens[(int64_t)2 * a.T * i + q] = nan;
    }
};

template <int W, int D, int HA = kActHiddenTanh, int OA = kActOutSoftplus>
struct SuppAdTan : SuppAd<W, D, HA, OA> {
    using Base = SuppAd<W, D, HA, OA>;
    using typename Base::Net;
    static constexpr int NS = 5, NERR = 3;          // [u1, u2, u3, du2, du3]: state 1 depends on no parameter
    using Args = SuppSensArgs;
    double dc[W];
    double info, score;
    __device__ __forceinline__ double init(const Args& a, double*, int, int64_t i, int64_t set, double (&y)[NS]) {
        double y3[3];
        const double chk = Base::init(a, nullptr, 0, i, set, y3);
        y[0] = y3[0]; y[1] = y3[1]; y[2] = y3[2]; y[3] = 0.0; y[4] = 0.0;
        Net::cond_tangent(this->p, exp(a.cond[set * a.set_stride_cond + i]), dc);
        info = score = 0.0;
        return chk;
    }
    __device__ __forceinline__ void rhs(int, double, const double (&Y)[NS], double (&du)[NS]) const {
        const double x[3] = {Y[0], Y[1], Y[2]}, dx[3] = {0.0, Y[3], Y[4]};
        double duh;
        const double uh = Net::template eval_jvp<true>(this->p, this->c, x, dc, dx, &duh);
        du[0] = -0.4 * Y[0];
        du[1] = fma(0.4, Y[0], -uh);
        du[2] = fma(-0.3, Y[2], uh);
        du[3] = -duh;
        du[4] = fma(-0.3, Y[4], duh);
    }
    __device__ __forceinline__ double residual2(const Args& a, int oi, int64_t i, const double (&o)[NS], bool active) {
        if (a.out.sens != nullptr && active) {
            double* tr = a.out.sens + (int64_t)3 * (oi + (int64_t)a.T * i);
            tr[0] = 0.0;
            tr[1] = o[3];
            tr[2] = o[4];
        }
        double s2 = 0.0;
#pragma unroll
        for (int s = 0; s < 3; s++) {
            const double r = o[s] - a.data[((int64_t)s * a.T + oi) * a.N + i];
            s2 = fma(r * a.iscale2[s], r, s2);
            if (s > 0) {
                info = fma(o[2 + s] * a.iscale2[s], o[2 + s], info);
                score = fma(r * a.iscale2[s], o[2 + s], score);
            }
        }
        return s2;
    }
    __device__ __forceinline__ void record(const Args& a, int64_t slot, int n, double t, double dt, const double (&y)[NS]) const {
        if (a.tape == nullptr || n >= a.tape_cap) return;
        double* e = a.tape + (int64_t)n * kSuppTapeRows * a.N + slot;
        e[0] = t;
        e[a.N] = dt;
#pragma unroll
        for (int s = 0; s < 3; s++) e[(2 + s) * a.N] = y[s];
    }
    __device__ __forceinline__ void finish(const Args& a, int64_t i, bool active, bool bad) const {
        if (!active) return;
        const double nan = __builtin_nan("");
        if (a.out.info != nullptr) a.out.info[i] = bad ? nan : info;
        if (a.out.score != nullptr) a.out.score[i] = bad ? nan : score;
        if (bad && a.out.sens != nullptr)
            for (int q = 0; q < 3 * a.T; q++) a.out.sens[(int64_t)3 * a.T * i + q] = nan;
    }
};

// ---------------------------------------------------------------------------------- order-2 policies (cude_curvature)
// The tangent policies carried one Taylor coefficient further: the state vector is [u; du; d2u], the right-hand side of
// the third part is the second-order tangent one (Net::eval_jet2), NERR is unchanged -- the accepted steps stay
// cude_forward's and the result is the second derivative of the accepted-step map.  The primal and first-order operations
// are those of CpepAdTan / SuppAdTan in the same order.
template <class Net>
struct CpepAdCurv : CpepAd<Net> {
    using Base = CpepAd<Net>;
    static constexpr int NS = 6, NERR = 2;          // [u1, u2, du1, du2, d2u1, d2u2]
    static constexpr int WAVES = 1;                 // (2-8-3: 220 bytes of scratch in a 256-register budget)
    using Args = CpepCurvArgs;
    double dc[Net::NCST], d2c[Net::NCST];
    double dbase, d2base, prod_last, dprod_last, d2prod_last, info, score, curv2;
    __device__ __forceinline__ double init(const Args& a, double* s_extra, int lane_, int64_t i, int64_t set, double (&y)[NS]) {
        double y2[2];
        const double chk = Base::init(a, s_extra, lane_, i, set, y2);
        y[0] = y2[0]; y[1] = y2[1];
#pragma unroll
        for (int s = 2; s < NS; s++) y[s] = 0.0;
        Net::cond_tangent(this->p, this->cst0, dc);
        Net::cond_tangent2(this->p, this->cst0, d2c);
        dbase = d2base = prod_last = dprod_last = d2prod_last = info = score = curv2 = 0.0;
        return chk;
    }
    __device__ __forceinline__ void rhs(int st, double te, const double (&Y)[NS], double (&du)[NS]) {
        // (stage 7 reuses stage 6's value, and the baseline comes first at st == -2: CpepAdTan::rhs)
        if (st != 6) {
            const int nr = st == -2 ? 2 : 1;
#pragma unroll 1
            for (int r = 0; r < nr; r++) {
                const bool is_base = st == -2 && r == 0;
                const double xx[1] = {is_base ? 0.0 : this->forcing_input(te)}, dx[1] = {0.0};
                double dv, d2v;
                const double v = Net::template eval_jet2<false>(this->p, this->c, xx, dc, dx, d2c, dx, &dv, &d2v);
                if (is_base) { this->base = v; dbase = dv; d2base = d2v; }
                else { prod_last = v; dprod_last = dv; d2prod_last = d2v; }
            }
        }
        du[0] = fma(this->a11, Y[0], fma(this->a12, Y[1], this->f0 + (prod_last - this->base)));
        du[1] = fma(this->a21, Y[0], this->a22 * Y[1]);
        du[2] = fma(this->a11, Y[2], fma(this->a12, Y[3], dprod_last - dbase));
        du[3] = fma(this->a21, Y[2], this->a22 * Y[3]);
        du[4] = fma(this->a11, Y[4], fma(this->a12, Y[5], d2prod_last - d2base));
        du[5] = fma(this->a21, Y[4], this->a22 * Y[5]);
    }
    __device__ __forceinline__ double residual2(const Args& a, int oi, int64_t i, const double (&o)[NS], bool active) {
        if (a.out2.sens2 != nullptr && active) {
            double* tr = a.out2.sens2 + (int64_t)2 * (oi + (int64_t)a.T * i);
            tr[0] = o[4];
            tr[1] = o[5];
        }
        const double r = o[0] - a.obs[(int64_t)oi * a.N + i];
        info = fma(o[2], o[2], info);
        score = fma(r, o[2], score);
        curv2 = fma(r, o[4], curv2);
        return r * r;
    }
    __device__ __forceinline__ void record(const Args& a, int64_t slot, int n, double, double dt, const double (&)[NS]) const {
        if (a.tape != nullptr && n < a.tape_cap) a.tape[(int64_t)n * a.N + slot] = dt;
    }
    __device__ __forceinline__ void finish(const Args& a, int64_t i, bool active, bool bad) const {
        if (!active) return;
        const double nan = __builtin_nan("");
        if (a.out.info != nullptr) a.out.info[i] = bad ? nan : info;
        if (a.out.score != nullptr) a.out.score[i] = bad ? nan : score;
        if (a.out2.curv != nullptr) a.out2.curv[i] = bad ? nan : info + curv2;
        if (bad && a.out2.sens2 != nullptr)
            for (int q = 0; q < 2 * a.T; q++) a.out2.sens2[(int64_t)2 * a.T * i + q] = nan;
    }
};

template <int W, int D, int HA = kActHiddenTanh, int OA = kActOutSoftplus>
struct SuppAdCurv : SuppAd<W, D, HA, OA> {
    using Base = SuppAd<W, D, HA, OA>;
    using typename Base::Net;
    static constexpr int NS = 7, NERR = 3;          // [u1, u2, u3, du2, du3, d2u2, d2u3]: state 1 depends on no parameter
    static constexpr int WAVES = 1;                 // (8-2: 188 bytes of scratch in a 256-register budget)
    using Args = SuppCurvArgs;
    double dc[W], d2c[W];
    double info, score, curv2;
    __device__ __forceinline__ double init(const Args& a, double*, int, int64_t i, int64_t set, double (&y)[NS]) {
        double y3[3];
        const double chk = Base::init(a, nullptr, 0, i, set, y3);
        y[0] = y3[0]; y[1] = y3[1]; y[2] = y3[2];
#pragma unroll
        for (int s = 3; s < NS; s++) y[s] = 0.0;
        const double cst0 = exp(a.cond[set * a.set_stride_cond + i]);
        Net::cond_tangent(this->p, cst0, dc);
        Net::cond_tangent2(this->p, cst0, d2c);
        info = score = curv2 = 0.0;
        return chk;
    }
    __device__ __forceinline__ void rhs(int, double, const double (&Y)[NS], double (&du)[NS]) const {
        const double x[3] = {Y[0], Y[1], Y[2]}, dx[3] = {0.0, Y[3], Y[4]}, d2x[3] = {0.0, Y[5], Y[6]};
        double duh, d2uh;
        const double uh = Net::template eval_jet2<true>(this->p, this->c, x, dc, dx, d2c, d2x, &duh, &d2uh);
        du[0] = -0.4 * Y[0];
        du[1] = fma(0.4, Y[0], -uh);
        du[2] = fma(-0.3, Y[2], uh);
        du[3] = -duh;
        du[4] = fma(-0.3, Y[4], duh);
        du[5] = -d2uh;
        du[6] = fma(-0.3, Y[6], d2uh);
    }
    __device__ __forceinline__ double residual2(const Args& a, int oi, int64_t i, const double (&o)[NS], bool active) {
        if (a.out2.sens2 != nullptr && active) {
            double* tr = a.out2.sens2 + (int64_t)3 * (oi + (int64_t)a.T * i);
            tr[0] = 0.0;
            tr[1] = o[5];
            tr[2] = o[6];
        }
        double s2 = 0.0;
#pragma unroll
        for (int s = 0; s < 3; s++) {
            const double r = o[s] - a.data[((int64_t)s * a.T + oi) * a.N + i];
            s2 = fma(r * a.iscale2[s], r, s2);
            if (s > 0) {
                info = fma(o[2 + s] * a.iscale2[s], o[2 + s], info);
                score = fma(r * a.iscale2[s], o[2 + s], score);
                curv2 = fma(r * a.iscale2[s], o[4 + s], curv2);
            }
        }
        return s2;
    }
    __device__ __forceinline__ void record(const Args& a, int64_t slot, int n, double t, double dt, const double (&y)[NS]) const {
        if (a.tape == nullptr || n >= a.tape_cap) return;
        double* e = a.tape + (int64_t)n * kSuppTapeRows * a.N + slot;
        e[0] = t;
        e[a.N] = dt;
#pragma unroll
        for (int s = 0; s < 3; s++) e[(2 + s) * a.N] = y[s];
    }
    __device__ __forceinline__ void finish(const Args& a, int64_t i, bool active, bool bad) const {
        if (!active) return;
        const double nan = __builtin_nan("");
        if (a.out.info != nullptr) a.out.info[i] = bad ? nan : info;
        if (a.out.score != nullptr) a.out.score[i] = bad ? nan : score;
        if (a.out2.curv != nullptr) a.out2.curv[i] = bad ? nan : info + curv2;
        if (bad && a.out2.sens2 != nullptr)
            for (int q = 0; q < 3 * a.T; q++) a.out2.sens2[(int64_t)3 * a.T * i + q] = nan;
    }
};

__device__ __forceinline__ double rms(const double* v, int n) {
    double s = 0.0;
    for (int k = 0; k < n; k++) s = fma(v[k], v[k], s);
    return sqrt(s / n);
}

// waves per SIMD the register allocation aims at: the solve is a latency chain, so a second resident wave is worth more
// than unrolling room, as long as the gradient accumulators (2 VGPRs each) leave space for it
// (a policy with a member WAVES names its own: the order-2 policies, whose widest shapes spill at two)
template <class M, class = void>
struct AdWaves {
    static constexpr int value = 0;
};
template <class M>
struct AdWaves<M, decltype((void)M::WAVES)> {
    static constexpr int value = M::WAVES;
};
template <class M, bool GRAD>
constexpr int adaptive_waves() {
    if (AdWaves<M>::value > 0) return AdWaves<M>::value;
    return !GRAD ? 2 : (M::NetT::NACC <= (M::NEED_Y ? 24 : CUDE_ADAPT_2W_NACC) ? 2 : 1);
}

// ---------------------------------------------------------------------------------- shared by the integrators
// weight of stage derivative j in the `saveat` output at theta = (t_out - t_n) / dt_n: Tsit5's free 4th-order interpolant,
// or -- at the end of the step -- the last tableau row (y_{n+1} itself)
__device__ __forceinline__ double saveat_weight(int j, double th, bool at_end) {
    return at_end ? (j < 6 ? TS_A[6][j < 6 ? j : 0] : 0.0)
                  : fma(fma(fma(TS_R[j][3], th, TS_R[j][2]), th, TS_R[j][1]) * th, th, TS_R[j][0] * th);
}

// OrdinaryDiffEq's PI controller (beta1 = 7/50, beta2 = 2/25, gamma = 0.9, qmin = 0.2, qmax = 10) on the scaled error
// estimate of a trial step.  q = est^(7/50) / qold^(2/25) with qold = max(previous est, 1e-4): both powers come from ONE
// logarithm per trial step -- est^(7/50) = exp(0.14 log est) now, and, when the step is accepted, qold^(2/25) of the
// NEXT step = exp(0.08 max(log est, log 1e-4)), carried in qold_pow (the two pow() calls per trial step were ~10 % of the
// forward sweep's instructions in round 2)
struct StepController {
    double qold_pow = 0.47863009232263831;         // (1e-4)^(2/25)
    double log_est = 0.0, q11 = 0.0;
    __device__ __forceinline__ bool judge(double est) {            // true: the step is accepted
        log_est = est > 0.0 ? log(est) : -1e3;                      // (est = 0: qold = 1e-4 below)
        q11 = est > 0.0 ? exp((7.0 / 50.0) * log_est) : 1e-12;
        return est <= 1.0;
    }
    __device__ __forceinline__ double after_accept(double dt) {    // the next step's size
        double q = q11 / qold_pow;
        q = fmax(1.0 / 10.0, fmin(1.0 / 0.2, q / 0.9));
        qold_pow = exp((2.0 / 25.0) * fmax(log_est, -9.21034037197618273607));     // log 1e-4
        return dt / q;
    }
    __device__ __forceinline__ double after_reject(double dt) const { return dt / fmin(1.0 / 0.2, q11 / 0.9); }
};

// a step's seven stage rows (derivatives, inputs or adjoints) in the unrolled kernels: registers (indices are literals
// after unrolling), or one LDS row each at a constant offset
template <int NS, bool IN_LDS>
struct StageRows {
    double v[7][NS];
    __device__ __forceinline__ StageRows(double*, int) {}
    __device__ __forceinline__ double get(int j, int s) const { return v[j][s]; }
    __device__ __forceinline__ void set(int j, int s, double x) { v[j][s] = x; }
};
template <int NS>
struct StageRows<NS, true> {
    double* row;
    __device__ __forceinline__ StageRows(double* rows, int lane) : row(rows + lane) {}
    __device__ __forceinline__ double get(int j, int s) const { return row[(j * NS + s) * kBlock]; }
    __device__ __forceinline__ void set(int j, int s, double x) { row[(j * NS + s) * kBlock] = x; }
};

constexpr int kUnrolledKnots = 5;                  // the reference's five sampling times (c-peptide/02-conditional.jl)
// cude_adaptive_unrolled.hip: the c-peptide MLP shapes (cude_shapes.h CUDE_CPEP_SHAPES) and the symbolic model on grids of at most kUnrolledKnots times; hipErrorNotSupported
// for any other shape (the caller then runs the phase-machine kernel)
hipError_t launch_cpep_adaptive_unrolled(const NetShape& net, bool grad, const CpepArgs& a, hipStream_t s);
// cude_adaptive_team.hip: the same solve with a step's five network evaluations on five waves, for launches of at most
// kTeamMaxWaves single-wave workgroups (the reference's own population sizes); hipErrorNotSupported otherwise
constexpr int kTeamMaxWaves = 256;
hipError_t launch_cpep_adaptive_team(const NetShape& net, bool grad, const CpepArgs& a, hipStream_t s);
// shape groups 1 and 2 of either integrator (their own translation units); hipErrorNotSupported = not in this group
hipError_t launch_cpep_adaptive_unrolled_part1(const NetShape& net, bool grad, const CpepArgs& a, hipStream_t s);
hipError_t launch_cpep_adaptive_unrolled_part2(const NetShape& net, bool grad, const CpepArgs& a, hipStream_t s);
hipError_t launch_cpep_adaptive_part1(const NetShape& net, bool grad, const CpepArgs& a, hipStream_t s);
hipError_t launch_cpep_adaptive_part2(const NetShape& net, bool grad, const CpepArgs& a, hipStream_t s);
// cude_adaptive_unrolled_supp.hip: the suppression model, shapes of the reference's experiments (cude_shapes.h
// CUDE_SUPP_AD_UNROLLED)
hipError_t launch_supp_adaptive_unrolled(const NetShape& net, bool grad, const SuppArgs& a, hipStream_t s);

}  // namespace cude
