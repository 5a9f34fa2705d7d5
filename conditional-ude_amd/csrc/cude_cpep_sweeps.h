// The two sweeps of the fixed-step c-peptide kernel -- forward solve, then (GRAD) the discrete adjoint -- as the TEXT of a
// function body.  cude_cpep.hip includes it twice: as the body of cpep_kernel itself, for the kernels that run one form
// of it, and as the body of cpep_sweeps<..., LEAN>, for the gradient kernels of the lean shapes, which hold a clamp-free
// and a clamped form and pick one per wave.  Text, not a shared function, so that the first group are the kernels they
// were: handed their argument block through a function, every one of them allocates its registers differently
// (profiles/lean_clamp.txt; profiles/adaptive_step_shared.txt for the same finding in the adaptive kernels).
// The includer provides: Net, NS, GRAD, KEEP, ROWS (the kernel's template parameters), CpepArgs a (an lvalue),
// constexpr bool LEAN (layers above the first and the output unit without their clamps, in both sweeps) and
// constexpr bool kSafeAnchor (tab_anchor without its clamps: dead behind tab_safe whatever the weights).
// No include guard, nothing but the body.
    constexpr int P = Net::P;
    constexpr int NC = Net::NC;
    constexpr int TABROWS = Net::HAS_TAB ? 5 * Net::NCST : 0;
    constexpr int REDROWS = TABROWS > kRedRows ? TABROWS : kRedRows;
    extern __shared__ double smem[];
    double* s_q = smem;                         // [5][kBlock] stage forcings (fwd) / adjoint weights (rev)
    double* s_red = smem + 5 * kBlock;          // [kRedRows][kBlock], only used after the time loops ...
    double* s_tab = s_red;                      // ... which use the same rows as [5][W][kBlock] layer-1 factor table
    double* s_res = s_red + REDROWS * kBlock;   // [T][kBlock] residuals kept for the reverse sweep

    const int lane = threadIdx.x;
    const int64_t gid = ((int64_t)blockIdx.x + (GRAD ? 0 : a.blk_first)) * kBlock + lane;
    const bool active = gid < a.N;
    const int64_t i = active ? gid : a.N - 1;
    const int64_t N = a.N;
    // multi-start screening: blockIdx.y selects one of n_sets (network, conditional) parameter sets
    const int64_t set = blockIdx.y;
    // (dense output of several sets, forward launches only: set k's trajectories start traj_set_stride further on)
    if constexpr (!GRAD) { if (a.traj != nullptr) a.traj += set * a.traj_set_stride; }
    cptr_t p = as_const(a.nn + set * a.set_stride_nn);
    cptr_t phi = as_const(a.phi);
    cptr_t obs_w = as_const(a.obs_w);
    ciptr_t seg = as_const(a.seg);
    ciptr_t obs_step = as_const(a.obs_step);
    const int S = a.S, T = a.T;
    const double h = a.h;

    const double k0 = a.k0[i], k1 = a.k1[i], k2 = a.k2[i], c0 = a.c0[i];
    const double a11 = -(k0 + k2), a12 = k1, a21 = k2, a22 = -k1, f0 = k0 * c0;
    // kept activations: one contiguous stretch per workgroup, [evaluation][value][lane] -- the wave streams through it
    // forwards, then backwards (the population-wide [value][subject] rows of the other buffers would scatter every
    // evaluation's 512-byte pieces a megabyte apart: measured 3.6 TB/s)
    constexpr int NK = KEEP == 2 ? Net::NKEEP : 1;            // kept values per evaluation (KEEP = 1: the logistic derivative)
    double* const act = KEEP ? a.act + (int64_t)blockIdx.x * ((int64_t)(5 * a.S + 1) * NK * kBlock) + lane : nullptr;
    double cst[NC];
    cst[0] = Net::cond_input(a.cond[set * a.set_stride_cond + i]);
    if (NC > 1) cst[1] = a.age[i];
    double c[Net::NCST];
    Net::first_layer_offset(p, cst, c);

#ifdef CUDE_WAVE_TIMING
    const long long dbg_t0 = wall_clock64();
    long long dbg_t1 = 0;
#endif
    // ------------------------------------------------------------------ forward
    double y1 = c0, y2 = (k2 / k1) * c0, y3 = 0.0;
    double qprev = 0.0;                          // q(t_0) = NN(0,.) - NN(0,.) == 0
    double K1a = fma(a11, y1, fma(a12, y2, f0)); // k_1 of the current step (FSAL)
    double K1b = fma(a21, y1, a22 * y2);
    int cur_seg = -1;
    double g_lo = 0.0, g_d = 0.0;
    double sse = 0.0, base = 0.0;
    double chk = fma(cst[0], 0.0, Net::param_check(p));   // NaN iff a parameter / beta is non-finite
    if (NC > 1) chk = fma(cst[1], 0.0, chk);
    int oi = 0;
    // One network call site: evaluation e = -1 is the baseline NN([0; e^beta]); e = 5n+s is the
    // s-th distinct stage time of step n.  After the 5th evaluation of a step the (state-only)
    // Runge-Kutta algebra of that step runs.
    int n = 0, s = -1;
    // layer-1 exponent table (Mlp only): anchor A_j = exp(2 z_j(t_n)), factors in s_tab
    ciptr_t stepk = as_const(a.stepk);
    cptr_t stepd = as_const(a.stepd);
    typename Net::Exps A, E1;
    int kind = 0;
    bool run_ok = false;                         // wave-uniform: the current run is inside the table's exact range
#ifndef CUDE_NO_VW
    constexpr bool kVW = (GRAD && Net::HAS_VW) || KEEP != 0;   // only where the reverse sweep already pays for the registers
#else
    constexpr bool kVW = false;
#endif
    typename Net::VW vw;
    if constexpr (kVW) Net::load_vw(p, vw);
    // Issue priority (CpepArgs::prio_shift > 0; single-round launches with two waves per SIMD): the arbiter serves the
    // OLDEST ready wave first, so of two co-resident waves one runs ahead, finishes at ~0.7 of the launch and leaves the
    // other alone on the SIMD at the poor single-wave issue rate.  The two take turns at the higher priority instead --
    // by the parity of their hardware wave slot, every 2^prio_shift evaluations -- and finish together
    // (125 000 subjects: 0.582 -> 0.554 ms; no effect with one wave per SIMD, -2 % over many rounds: off there).
    //
    // WHEN the turns change (CpepArgs::prio_clock).  0: by each wave's own progress, as above.  The two waves are then
    // complementary only while they are in step; once one is ahead there is a stretch in every period where both hold
    // the same priority, age decides, and it decides for the same wave again.  k > 0: by the shader clock both waves
    // read -- high priority while bit k of s_memtime differs from the slot parity -- so that the two are complementary
    // at every instant, wherever each stands in its own sweep (125 000 subjects, timeline of the pairs: the earlier
    // wave of a pair leaves 0.22 of the launch before the other with the progress-keyed turns, 0.026 with k = 17;
    // 0.523 -> 0.494 ms, flat over k = 16 ... 19: profiles/prio_clock.txt).  The clock is requested next to seg[e] / phi[e] and
    // comes back with them: one scalar round trip, no wait of its own.  One register carries both forms: prio > 0 is
    // the progress-keyed shift, prio < 0 the clock bit under a set sign bit.  The adaptive kernels (cude_adaptive_body.h,
    // cude_adaptive_unrolled.hip) carry the progress-keyed form only: their work per wave is data-dependent, and the
    // host never hands them a clock bit (run_ensemble).
    const unsigned prio_par = GRAD ? (__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (3 << 11)) & 1u) : 0u;   // HW_ID.wave_id
    const int prio = !GRAD || a.prio_shift <= 0 ? 0 : (a.prio_clock > 0 ? (int)(0x80000000u | (unsigned)a.prio_clock) : a.prio_shift);
    // (every test looks at `prio` through an empty asm of its own, so that it stays the ONE scalar register the
    // progress-keyed form had.  Left to itself the compiler keeps the outcome of the mode tests and the shift count in
    // five more, across the loops, which the reverse sweep does not have: they come back as lane reads in the
    // evaluation blocks.)
    auto prio_now = [&]() {
        int v = prio;
        asm volatile("" : "+s"(v));
        return v;
    };
    auto prio_by_clock = [&](uint64_t t) {
        if (((unsigned)(t >> (prio_now() & 63)) ^ prio_par) & 1u) __builtin_amdgcn_s_setprio(2);
        else __builtin_amdgcn_s_setprio(0);
    };
    // (here, not at the top: the table's global read then travels with the subject's own loads -- one latency, not two)
    if constexpr (Net::USES_TANH) tanh_tab_init(lane, !Net::LDS_BIAS);
    Net::bias_init(a.nn + set * a.set_stride_nn, lane);
    // (the baseline evaluation e = -1 has no scalar loads for the clock to travel with: its turn is set here, with a
    // wait of its own, once per wave -- not in an else-arm of `if (e >= 0)` below, which changes how the loop's values
    // merge: ~20 more register copies per evaluation, the whole launch 4 % slower in EVERY mode)
    if (GRAD && prio_now() < 0) prio_by_clock(__builtin_amdgcn_s_memtime());
#pragma unroll 1
    for (int e = -1; e < 5 * S; e++) {
        if (const int pr = GRAD ? prio_now() : 0; pr > 0) {
            if ((((unsigned)(e + 1) >> pr) ^ prio_par) & 1u) __builtin_amdgcn_s_setprio(2);
            else __builtin_amdgcn_s_setprio(0);
        }
        double xv = 0.0;
        bool tab = false;
        if (e >= 0) {
            uint64_t clk = 0;
            if (GRAD && prio_now() < 0) clk = __builtin_amdgcn_s_memtime();
            const int sg = seg[e];
            const double ph = phi[e];     // requested together with seg[e]: one scalar round trip, not two
            if (GRAD && prio_now() < 0) prio_by_clock(clk);      // (the clock has come back with them)
            if (sg != cur_seg) {                 // wave-uniform: a handful of times per trajectory
                cur_seg = sg;
                g_lo = a.dG[(int64_t)sg * N + i];
                g_d = a.dG[(int64_t)(sg + 1) * N + i] - g_lo;
                chk = fma(g_d, 0.0, fma(g_lo, 0.0, chk));
            }
            xv = fma(ph, g_d, g_lo);
            if constexpr (Net::HAS_TAB) {
                if (s == 0) {                    // first evaluation of step n
                    kind = stepk[3 * n];
                    if (kind == 2 && !run_ok) kind = 0;
                    if (kind == 1) {             // a run of steps inside one glucose piece starts here
                        const int s0 = stepk[3 * n + 2];
                        const double lo = a.dG[(int64_t)s0 * N + i];
                        const double d = a.dG[(int64_t)(s0 + 1) * N + i] - lo;
                        run_ok = !__any(!Net::tab_safe(p, c, lo, d, stepd[3 * n + 2]));
                        if (run_ok) {
                            const double cf[5] = {Tab::c(1), Tab::c(2), Tab::c(3), Tab::c(4), 1.0};
                            Net::tab_build(p, d * stepd[3 * n + 2], cf, s_tab, lane);
                            Net::template tab_anchor<kSafeAnchor>(p, c, fma(stepd[3 * n], d, lo), A);
                        } else {
                            kind = 0;
                        }
                    } else if (kind == 2) {
#pragma unroll
                        for (int j = 0; j < Net::NCST; j++) A.v[j] *= s_tab[(4 * Net::NCST + j) * kBlock + lane];
                    }
                }
                tab = kind != 0;
                if (tab) {
#pragma unroll
                    for (int j = 0; j < Net::NCST; j++) E1.v[j] = A.v[j] * s_tab[(s * Net::NCST + j) * kBlock + lane];
                }
            }
        }
        const double x[1] = {xv};
        double v;
        if constexpr (KEEP == 2) {
            double keep[Net::NKEEP];
            v = Net::eval_vw_keep(p, vw, c, x, tab, &E1, keep);
            double* dst = act + (int64_t)(e + 1) * (Net::NKEEP * kBlock);
#pragma unroll
            for (int q = 0; q < Net::NKEEP; q++) dst[q * kBlock] = keep[q];
        } else if constexpr (KEEP == 1) {
            double sg;
            v = Net::eval_vw_sig(p, vw, c, x, tab, &E1, &sg);
            act[(int64_t)(e + 1) * kBlock] = sg;
        } else if constexpr (LEAN) {
            if constexpr (kVW) v = Net::template eval_vw<true>(p, vw, c, x, tab, &E1);
            else v = Net::template eval<true>(p, c, x, tab, &E1);
        } else if constexpr (kVW) {
            v = Net::eval_vw(p, vw, c, x, tab, &E1);
        } else {
            v = Net::eval(p, c, x, tab, &E1);
        }
        if (e < 0) { base = v; s = 0; continue; }
        s_q[s * kBlock + lane] = v - base;
        if (++s < 5) continue;
        s = 0;
        // ---- step n
        double q[7];
        q[0] = qprev;
#pragma unroll
        for (int j = 0; j < 5; j++) q[j + 1] = s_q[j * kBlock + lane];
        q[6] = q[5];
        double K[7][2];
        K[0][0] = K1a;
        K[0][1] = K1b;
        double Y1 = y1, Y2 = y2;
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
            K[st][0] = fma(a11, Y1, fma(a12, Y2, f0 + q[st]));   // st = 6: k7 = f(t_{n+1}, y_{n+1})
            K[st][1] = fma(a21, Y1, a22 * Y2);
        }
        double y3n = y3;
        if (NS == 3) {
            double t3 = 0.0;
#pragma unroll
            for (int j = 0; j < 6; j++) t3 = fma(Tab::a(6, j), q[j], t3);
            y3n = fma(h, t3, y3);
        }
        while (oi < T && obs_step[oi] == n) {
            double o1 = 0.0, o2 = 0.0, o3 = 0.0;
#pragma unroll
            for (int j = 0; j < 7; j++) {
                const double w = obs_w[oi * 7 + j];
                o1 = fma(w, K[j][0], o1);
                o2 = fma(w, K[j][1], o2);
                if (NS == 3) o3 = fma(w, q[j], o3);
            }
            o1 = fma(h, o1, y1);
            o2 = fma(h, o2, y2);
            o3 = fma(h, o3, y3);
            const double r = a.obs != nullptr ? o1 - a.obs[(int64_t)oi * N + i] : 0.0;   // null: cude_simulate
            sse = fma(r, r, sse);
            if (GRAD) s_res[oi * kBlock + lane] = r;
            // (unit adjoint seed, CpepArgs::unit_seed: the reverse sweep reads 1.0 / 0.0 where it read the residual)
            if constexpr (ROWS) { if (a.unit_seed > 0) s_res[oi * kBlock + lane] = unit_seed_cpep(a, set, oi); }
            if (a.traj != nullptr && active) {
                double* tr = a.traj + (int64_t)NS * (oi + (int64_t)T * i);
                tr[0] = o1;
                tr[1] = o2;
                if (NS == 3) tr[2] = o3;
            }
            oi++;
        }
        y1 = Y1;
        y2 = Y2;
        y3 = y3n;
        K1a = K[6][0];
        K1b = K[6][1];
        qprev = q[6];
        n++;
    }
    sse += chk;
#ifdef CUDE_WAVE_TIMING
    dbg_t1 = wall_clock64();
#endif
    const bool failed = !(fabs(sse) <= 1.79769313486231570815e308);   // NaN or Inf
    if (active) {
        if (a.sse != nullptr) a.sse[set * a.set_stride_cond + i] = sse;
        if (NS == 3 && a.auc != nullptr) a.auc[i] = y3;
    }
    const double red_loss = active ? sse : 0.0;
    const double red_fail = (active && failed) ? 1.0 : 0.0;
    double* out = a.partials + ((int64_t)set * gridDim.x + blockIdx.x) * (P + 2);

    if (!GRAD) {
        const double v2[2] = {red_loss, red_fail};
        block_reduce_store<2>(v2, s_red, out + P, lane);
        return;
    } else {
        // -------------------------------------------------------------- reverse sweep
        double acc[Net::NACC];
#pragma unroll
        for (int q = 0; q < Net::NACC; q++) acc[q] = 0.0;
        // the hidden layer of this launch row's parameter set, held in SGPRs for all 5 S + 1 reverse evaluations
#ifndef CUDE_NO_RW
        constexpr bool kRW = Net::HAS_RW && KEEP == 0;
#else
        constexpr bool kRW = false;
#endif
        typename Net::RW rw;
        if constexpr (kRW) Net::load_rw(a.nn + set * a.set_stride_nn, lane, rw);
        double dxdummy[1] = {0.0};
        double lam1 = 0.0, lam2 = 0.0;       // adjoint of y_{n+1}
        double kap1 = 0.0, kap2 = 0.0;       // adjoint of k_1 of step n+1 (= k_7 of step n)
        double wtot = 0.0;
        const double gscale = 2.0 * a.inv_n;
        oi = T - 1;
        cur_seg = -1;
        n = S - 1;
        s = 4;
        // kept activations of the evaluation about to be reversed, requested one evaluation ahead
        double kn[NK];
        if constexpr (KEEP != 0) {
            const double* src = act + (int64_t)(5 * S) * (NK * kBlock);
#pragma unroll
            for (int q = 0; q < NK; q++) kn[q] = src[q * kBlock];
        }
        // evaluations in reverse order; e = -1 is the baseline with weight -sum(w)
#pragma unroll 1
        for (int e = 5 * S - 1; e >= -1; e--) {
            if (const int pr = prio_now(); pr > 0) {
                if ((((unsigned)(e + 1) >> pr) ^ prio_par) & 1u) __builtin_amdgcn_s_setprio(2);
                else __builtin_amdgcn_s_setprio(0);
            }
                if (e >= 0 && s == 4) {
                // ---- adjoint algebra of step n (J_f = A, no forward state needed)
                double kb[7][2];
#pragma unroll
                for (int j = 0; j < 6; j++) { kb[j][0] = 0.0; kb[j][1] = 0.0; }
                kb[6][0] = kap1;
                kb[6][1] = kap2;
                double yb1 = 0.0, yb2 = 0.0;
                while (oi >= 0 && obs_step[oi] == n) {
                    double g = gscale * s_res[oi * kBlock + lane];
                    if constexpr (ROWS) { if (a.unit_seed > 0) g = s_res[oi * kBlock + lane]; }     // (a unit seed is taken as it is)
                    yb1 += g;
                    const double hg = h * g;
#pragma unroll
                    for (int j = 0; j < 7; j++) kb[j][0] = fma(obs_w[oi * 7 + j], hg, kb[j][0]);
                    oi--;
                }
                double w[5];
                // stage 7: k7 = A y_{n+1} + g7
                lam1 = fma(a11, kb[6][0], fma(a21, kb[6][1], lam1));
                lam2 = fma(a12, kb[6][0], fma(a22, kb[6][1], lam2));
                w[4] = kb[6][0];
                // y_{n+1} = y_n + h sum a7j k_j
                yb1 += lam1;
                yb2 += lam2;
                {
                    const double hl1 = h * lam1, hl2 = h * lam2;
#pragma unroll
                    for (int j = 0; j < 6; j++) {
                        kb[j][0] = fma(Tab::a(6, j), hl1, kb[j][0]);
                        kb[j][1] = fma(Tab::a(6, j), hl2, kb[j][1]);
                    }
                }
#pragma unroll
                for (int st = 5; st >= 1; st--) {
                    const double Yb1 = fma(a11, kb[st][0], a21 * kb[st][1]);
                    const double Yb2 = fma(a12, kb[st][0], a22 * kb[st][1]);
                    if (st == 5) w[4] += kb[5][0];
                    else w[st - 1] = kb[st][0];
                    yb1 += Yb1;
                    yb2 += Yb2;
                    const double h1 = h * Yb1, h2 = h * Yb2;
#pragma unroll
                    for (int j = 0; j < st; j++) {
                        kb[j][0] = fma(Tab::a(st, j), h1, kb[j][0]);
                        kb[j][1] = fma(Tab::a(st, j), h2, kb[j][1]);
                    }
                }
                lam1 = yb1;
                lam2 = yb2;
                kap1 = kb[0][0];
                kap2 = kb[0][1];
#pragma unroll
                for (int j = 0; j < 5; j++) s_q[j * kBlock + lane] = w[j];
                if constexpr (Net::HAS_TAB) {
                    // reverse sweep: the anchor is exp(2 z_j) at the END of step n, factors reach back from there
                    kind = stepk[3 * n + 1];
                    if (kind == 2 && !run_ok) kind = 0;
                    if (kind == 1) {
                        const int s0 = stepk[3 * n + 2];
                        const double lo = a.dG[(int64_t)s0 * N + i];
                        const double d = a.dG[(int64_t)(s0 + 1) * N + i] - lo;
                        run_ok = !__any(!Net::tab_safe(p, c, lo, d, stepd[3 * n + 2]));
                        if (run_ok) {
                            const double cr[5] = {Tab::c(1) - 1.0, Tab::c(2) - 1.0, Tab::c(3) - 1.0, Tab::c(4) - 1.0,
                                                  -1.0};
                            Net::tab_build(p, d * stepd[3 * n + 2], cr, s_tab, lane);
                            Net::template tab_anchor<kSafeAnchor>(p, c, fma(stepd[3 * n + 1], d, lo), A);
                        } else {
                            kind = 0;
                        }
                    } else if (kind == 2) {
#pragma unroll
                        for (int j = 0; j < Net::NCST; j++) A.v[j] *= s_tab[(4 * Net::NCST + j) * kBlock + lane];
                    }
                }
                n--;
            }
            double xv = 0.0, wv;
            bool tab = false;
            typename Net::RS rs;
            if constexpr (kRW) Net::rw_request(p, rs);   // travels with seg[e] and phi[e]: one scalar round trip
            if (e >= 0) {                                // (the baseline, last of the sweep, keeps the turn it inherits)
                uint64_t clk = 0;
                if (prio_now() < 0) clk = __builtin_amdgcn_s_memtime();
                const int sg = seg[e];
                const double ph = phi[e];
                if (prio_now() < 0) prio_by_clock(clk);
                if (sg != cur_seg) {
                    cur_seg = sg;
                    g_lo = a.dG[(int64_t)sg * N + i];
                    g_d = a.dG[(int64_t)(sg + 1) * N + i] - g_lo;
                }
                xv = fma(ph, g_d, g_lo);
                wv = s_q[s * kBlock + lane];
                wtot += wv;
                if constexpr (Net::HAS_TAB) {
                    tab = kind != 0;
                    if (tab) {
                        // all W factors are requested together and unconditionally (left to itself the compiler
                        // branches on the wave-uniform s around every single read: six exposed LDS round trips)
                        const int sr = s < 4 ? s : 0;
                        double f[Net::NCST];
#pragma unroll
                        for (int j = 0; j < Net::NCST; j++) f[j] = s_tab[(sr * Net::NCST + j) * kBlock + lane];
#pragma unroll
                        for (int j = 0; j < Net::NCST; j++) asm volatile("" : "+v"(f[j]));
                        // s is wave-uniform: a branch, not a select per lane (written as a select, the compiler
                        // multiplies always and picks with two v_cndmask_b32 per unit; the pin on the copies keeps it
                        // from converting the branch back)
                        if (s < 4) {
#pragma unroll
                            for (int j = 0; j < Net::NCST; j++) E1.v[j] = A.v[j] * f[j];
                        } else {                 // stage 5 sits at the anchor time itself
#pragma unroll
                            for (int j = 0; j < Net::NCST; j++) {
                                E1.v[j] = A.v[j];
                                asm volatile("" : "+v"(E1.v[j]));
                            }
                        }
                    }
                }
                s = (s == 0) ? 4 : s - 1;
            } else {
                wv = -wtot;
            }
            const double x[1] = {xv};
            if constexpr (KEEP == 1) {
                const double sg = kn[0];
                if (e >= 0) kn[0] = act[(int64_t)e * kBlock];      // next evaluation's value: in flight during this one
                Net::template eval_grad_pf<false, decltype(acc), true>(p, c, x, wv, acc, dxdummy, tab, &E1, sg);
            } else if constexpr (KEEP == 2) {
                double hk[Net::DEPTH][Net::WIDTH];
#pragma unroll
                for (int l = 1; l < Net::DEPTH; l++)
#pragma unroll
                    for (int j = 0; j < Net::WIDTH; j++) hk[l][j] = kn[(l - 1) * Net::WIDTH + j];
                const double sg = kn[Net::NKEEP - 1];
                if (e >= 0) {                   // next evaluation's (e - 1: row block e) values: in flight during this one
                    const double* src = act + (int64_t)e * (Net::NKEEP * kBlock);
#pragma unroll
                    for (int q = 0; q < Net::NKEEP; q++) kn[q] = src[q * kBlock];
                }
                Net::layer1(p, c, x, hk[0], tab, &E1);
                Net::template backward<false>(launder(p), x, hk, sg, wv, acc, dxdummy);
            } else if constexpr (LEAN) {
                if constexpr (kRW) Net::template eval_grad_rw<decltype(acc), true>(p, rw, rs, c, x, wv, acc, tab, &E1);
                else Net::template eval_grad<false, decltype(acc), Net::kPinLayers, 0, true>(p, c, x, wv, acc, dxdummy, tab, &E1);
            } else if constexpr (kRW) {
                Net::eval_grad_rw(p, rw, rs, c, x, wv, acc, tab, &E1);
            } else {
                Net::template eval_grad<false>(p, c, x, wv, acc, dxdummy, tab, &E1);
            }
        }

        // Behind the sweep the whole dynamic allocation is dead (stage weights, factor table, residuals): where its
        // fixed part alone -- (5 + REDROWS) rows, whatever T (launch_one) -- holds the doubled rows, the reduction
        // reads them at constant offsets (block_reduce_expand_wide).  The other shapes allocate kRedRows rows only.
        constexpr bool kWide = 5 + REDROWS >= kRedWideRows;
        if constexpr (kRW) {
            // the subject index and exp(beta) are formed again here: carried through the sweep, their four registers
            // are the ones the resident layer needs
            int le = lane;
            asm volatile("" : "+v"(le));
            const int64_t ge = (int64_t)blockIdx.x * kBlock + le;
            const int64_t ie = ge < a.N ? ge : a.N - 1;
            double ce[NC];
            ce[0] = Net::cond_input(a.cond[set * a.set_stride_cond + ie]);
            if (active) a.g_cond[set * a.set_stride_cond + ie] = Net::grad_cond(p, acc, ce);
            if constexpr (ROWS) store_lane_rows<Net, NC>(acc, ce, active, a.lane_rows + (set * P) * N + ie, N);
            static_assert(kWide, "the resident-layer kernel has a factor table: 35 rows of LDS");
            block_reduce_expand_wide<Net, NC>(acc, ce, active ? 1.0 : 0.0, red_loss, red_fail, smem, out, lane);
        } else {
        if (active) a.g_cond[set * a.set_stride_cond + i] = Net::grad_cond(p, acc, cst);
        if constexpr (ROWS) store_lane_rows<Net, NC>(acc, cst, active, a.lane_rows + (set * P) * N + i, N);
        if constexpr (kWide) block_reduce_expand_wide<Net, NC>(acc, cst, active ? 1.0 : 0.0, red_loss, red_fail, smem, out, lane);
        else block_reduce_expand<Net, NC>(acc, cst, active ? 1.0 : 0.0, red_loss, red_fail, s_red, out, lane);
        }
#ifdef CUDE_WAVE_TIMING
        if (a.dbg != nullptr && lane == 0 && blockIdx.y == 0) {
            long long* d = a.dbg + 4 * (long long)blockIdx.x;
            d[0] = dbg_t0;
            d[1] = dbg_t1;
            d[2] = wall_clock64();
            d[3] = (long long)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11)) |      // HW_ID
                   ((long long)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11)) << 32);  // XCC_ID
        }
#endif
    }
