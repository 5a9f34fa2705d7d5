// libcude_hip.so -- the entry points that batch launches: dense output and predictive bands, conditional sets, marginal
// likelihoods, subject scores, network information, sensitivities, multi-start evaluation and screening, likelihood
// profiles and their intervals, per-subject fits.  Each is its own argument checks, chunking, small kernels and copies
// around the launches of cude_launch.hip, in chunks sized by cude_select.hip's sets_per_launch.  (The entry points that
// simulate replicates of the data: cude_replicates.hip.)
#include "cude_ctx.h"

using namespace cude::api;

namespace {
// Sets per eval_sets_device call of cude_subject_scores: the rows table ([P][N] per set) and the per-set rows of
// conditionals, weights, SSEs and conditional gradients next to the launch's own scratch (whose share of the budget
// eval_sets_device takes by itself, so half of the budget each); option "profile_chunk" > 0 lowers it.
int64_t scores_chunk_sets(cude_ctx* c, int64_t n_sets) {
    const double per_set = 8.0 * ((double)c->P + 4.0) * (double)c->N;
    return sets_per_launch(n_sets, 32768, 0.5 * sets_scratch_budget(c), per_set, c->opt.profile_chunk);
}

// Live outputs per eval_sets_device call of cude_network_information: as scores_chunk_sets, with the staging of the rows as
// [N][outputs][P] (up to 3 output rows per 2 live outputs) when the caller wants the Jacobian itself
int64_t info_chunk_sets(cude_ctx* c, int64_t n_live, bool stage) {
    const double per_set = 8.0 * ((stage ? 2.5 : 1.0) * (double)c->P + 3.0) * (double)c->N;
    return sets_per_launch(n_live, 32768, 0.5 * sets_scratch_budget(c), per_set, c->opt.profile_chunk);
}

// Grid points per launch of a likelihood-profile scan (cude_profile_conditional, cude_profile_intervals): the grid's y
// dimension and ~512 MB of scratch (conditional sets, SSEs, partial rows); option "profile_chunk" > 0 lowers it.
int64_t profile_chunk_sets(cude_ctx* c, int64_t n_points) {
    const double per_point = 8.0 * (2.0 * c->N + (double)c->nblocks * (c->P + 2));
    return sets_per_launch(n_points, 32768, 512e6, per_point, c->opt.profile_chunk);
}

// Dense output (cude_simulate, cude_predictive_bands): the output times must lie inside the population's time span and
// not decrease
int32_t check_output_times(const cude_ctx* c, int32_t n_times, const double* times) {
    const double t0 = c->tp.front(), t1 = c->tp.back(), h = adaptive(c) ? (t1 - t0) : (t1 - t0) / c->cfg.n_steps;
    for (int i = 0; i < n_times; i++) {
        if (!(times[i] >= t0 - 1e-9 * h && times[i] <= t1 + 1e-9 * h))
            return fail(CUDE_ERR_ARG, "output times must lie inside the time span of the population");
        if (i > 0 && !(times[i] >= times[i - 1])) return fail(CUDE_ERR_ARG, "output times must be non-decreasing");
    }
    return CUDE_OK;
}
}  // namespace

// The stepped form of the per-subject fits (cude_refine_conditional; one replicate of cude_bootstrap_conditional): per
// evaluation a tangent launch at the trial points and the rule's update; every round is queued, the subjects that have
// stopped keep their state (and are solved along at their last trial point).  obs_ov: launch_tangent's.
hipError_t cude::api::refine_stepped(cude_ctx* c, const cude::RefineCfg& k, const cude::RefineArrays& r, double* sse_t, double* score_t,
                                     double* info_t, const double* obs_ov) {
    hipError_t le = cude::launch_refine_step(0, k, r, c->stream);
    cude::SensOut out;
    out.info = info_t;
    out.score = score_t;
    for (int it = 0; it < k.max_evals && le == hipSuccess; it++) {
        le = launch_tangent(c, r.xt, sse_t, out, false, obs_ov);
        if (le == hipSuccess) le = cude::launch_refine_step(1, k, r, c->stream);
    }
    // (adaptive mode: nothing of these solves is on the gradient's tape -- cude_adaptive_steps refuses afterwards)
    note_adaptive_launch(c, false);
    return le;
}

// the search state of the fits in the context's scratch (13 rows of doubles, 2 of int32); x0 is the caller's
int32_t cude::api::refine_state(cude_ctx* c, cude::RefineArrays& r, double** sse_t, double** score_t, double** info_t) {
    const int64_t N = c->N;
    HIP_TRY(c->refine_buf.reserve((size_t)13 * N));       // x0, x, F, sse, info, g, lam, xp, gp, xt, sse_t, score_t, info_t
    HIP_TRY(c->refine_ibuf.reserve((size_t)2 * N));       // evals, status
    double* q = c->refine_buf.p;
    r.N = N;
    r.x = q + N; r.F = q + 2 * N; r.sse = q + 3 * N; r.info = q + 4 * N;
    r.g = q + 5 * N; r.lam = q + 6 * N; r.xp = q + 7 * N; r.gp = q + 8 * N; r.xt = q + 9 * N;
    *sse_t = q + 10 * N;
    *score_t = q + 11 * N;
    *info_t = q + 12 * N;
    r.sse_t = *sse_t; r.score_t = *score_t; r.info_t = *info_t;
    r.evals = c->refine_ibuf.p; r.status = c->refine_ibuf.p + N;
    return CUDE_OK;
}


// The device half of cude_network_information (rules 2 ... 7 there): the unit-seed launches and the fold, finish and cross
// kernels.  Leaves b, d, jc, qf and status (tb.ia), A (tb.gn, with want_a) and the Schur complement (tb.schur, with
// want_schur) on the device, in scratch of the context that the next call of this function reuses; writes rq.jac_out chunk
// by chunk; tb.failed is final after the next synchronisation of the stream.  The caller has checked the arguments.
int32_t cude::api::info_pass(cude_ctx* c, const InfoRequest& rq, InfoTables& tb) {
    int32_t rc = CUDE_OK;
    const int P = c->P;
    const int64_t N = c->N;
    const double* const cond = rq.cond;
    const double* const cov = rq.cov;
    double* const jac_out = rq.jac_out;
    const int profiled = rq.profiled ? 1 : 0;
    const bool cpep = is_cpep(c);
    const int T = c->T, n_out = cpep ? T : 3 * T;
    const int n_live = cpep ? T - 1 : 2 * (T - 1);
    const bool want_a = rq.want_a, want_q = rq.want_q;
    const int64_t chunk = n_live > 0 ? info_chunk_sets(c, n_live, jac_out != nullptr) : 1;
    const bool single = chunk >= n_live;
    const int span_max = cpep ? (int)chunk : 3 * (((int)chunk + 1) / 2) + 2;
    const size_t n_part = cude::info_cross_partials(N, P);
    // per-set rows of a launch: conditionals, SSEs, conditional gradients
    HIP_TRY(c->sc_rows.reserve((size_t)chunk * P * N));
    HIP_TRY(c->sc_sets.reserve((size_t)chunk * 3 * N));
    HIP_TRY(c->ms_out.reserve((size_t)chunk * (P + 2)));
    if (jac_out) HIP_TRY(c->ni_stage.reserve((size_t)N * span_max * P));
    double* const d_cond = c->sc_sets.p;
    double* const d_sse = d_cond + chunk * N;
    double* const d_gcond = d_sse + chunk * N;
    cude::InfoArgs& ia = tb.ia;
    ia = cude::InfoArgs{};
    ia.N = N; ia.P = P; ia.n_out = n_out; ia.supp = cpep ? 0 : 1;
    for (int s = 0; s < 3; s++) ia.w[s] = cpep ? 1.0 : 1.0 / (c->scale[s] * c->scale[s]);
    ia.pw = rq.pw;
    // state (b, t, d are cleared as one stretch, jc and qf as another; the kernels take status at bad + N)
    double *d_coup = nullptr, *d_cond0 = nullptr, *d_gn = nullptr, *d_x = nullptr, *d_schur = nullptr, *d_cov = nullptr,
           *d_part = nullptr, *d_partx = nullptr;
    int32_t* d_nfail = nullptr;
    HIP_TRY(carve(c->ni_state, [&](Carve<double>& v) {
        ia.b = v.take((size_t)P * N);           // [P][N]
        ia.t = v.take((size_t)P * N);
        ia.d = v.take(N);
        ia.jc = v.take((size_t)n_out * N);      // [N][n_out]
        ia.qf = v.take((size_t)n_out * N);
        d_coup = v.take((size_t)P * N);         // the coupling table as [N][P]
        d_cond0 = v.take(N);                    // the conditional vector
        d_gn = v.take((size_t)P * P);           // gn, the Schur term, schur, cov: [P][P]
        d_x = v.take((size_t)P * P);
        d_schur = v.take((size_t)P * P);
        d_cov = v.take((size_t)P * P);
        d_part = v.take(n_part);                // two sets of cross-product partials
        d_partx = v.take(n_part);
    }));
    HIP_TRY(carve(c->sc_int, [&](Carve<int32_t>& v) {
        ia.bad = v.take(N);
        ia.status = v.take(N);
        d_nfail = v.take(1);
    }));
    ia.mask = c->param_mask.p;
    const double* cond0 = c->cond.p;
    if (cond) {
        HIP_TRY(push(c, d_cond0, cond, N));
        cond0 = d_cond0;
    }
    HIP_TRY(cude::launch_info_replicate(N, (int)chunk, cond0, d_cond, c->stream));
    if (want_q) HIP_TRY(push(c, d_cov, cov, (size_t)P * P));
    // the rows of t_0 and of suppression state 0 depend on no parameter: +0.0 without a launch
    HIP_TRY(hipMemsetAsync(ia.jc, 0, (size_t)2 * n_out * N * sizeof(double), c->stream));
    if (jac_out) std::memset(jac_out, 0, (size_t)N * n_out * P * sizeof(double));
    SetsRows rows{c->sc_rows.p, d_sse, 0};
    const auto solve = [&](int l0, int kn) {
        rows.unit_seed = 1 + l0;
        return eval_sets_device(c, kn, c->nn.p, 0, d_cond, N, d_gcond, c->ms_out.p, &rows);
    };
    if (n_live == 0) {       // (a population with one time point: the fold of nothing)
        HIP_TRY(hipMemsetAsync(ia.b, 0, (size_t)(2 * P + 1) * N * sizeof(double), c->stream));
        HIP_TRY(hipMemsetAsync(ia.bad, 0, (size_t)N * sizeof(int32_t), c->stream));
        HIP_TRY(hipMemsetAsync(d_part, 0, n_part * sizeof(double), c->stream));
    }
    // ---- first pass: b, d, the failures; the caller's Jacobian chunk by chunk.  With several chunks A is summed along in
    // the hope that no subject fails (the second pass needs every launch again)
    const bool a_along = want_a && !single && !want_q;
    for (int l0 = 0; l0 < n_live; l0 += (int)chunk) {
        const int kn = (int)std::min<int64_t>(chunk, n_live - l0);
        if ((rc = solve(l0, kn))) return rc;
        HIP_TRY(cude::launch_info_fold(ia, kn, l0, l0 == 0, c->sc_rows.p, d_gcond, d_sse, c->stream));
        if (a_along) HIP_TRY(cude::launch_info_cross(ia, kn, l0, l0 == 0, c->sc_rows.p, nullptr, d_part, c->stream));
        if (jac_out) {
            const int o0 = ia.out_index(l0), span = ia.out_index(l0 + kn - 1) - o0 + 1;
            HIP_TRY(hipMemsetAsync(c->ni_stage.p, 0, (size_t)N * span * P * sizeof(double), c->stream));
            HIP_TRY(cude::launch_info_transpose(ia, kn, l0, span, c->sc_rows.p, true, c->ni_stage.p, c->stream));
            HIP_TRY(hipMemcpy2DAsync(jac_out + (size_t)o0 * P, (size_t)n_out * P * sizeof(double), c->ni_stage.p,
                                     (size_t)span * P * sizeof(double), (size_t)span * P * sizeof(double), (size_t)N,
                                     hipMemcpyDeviceToHost, c->stream));
        }
    }
    HIP_TRY(hipMemsetAsync(d_nfail, 0, sizeof(int32_t), c->stream));
    HIP_TRY(cude::launch_info_finish(ia, d_nfail, c->stream));
    int32_t& failed = tb.failed;
    failed = 0;
    HIP_TRY(fetch(c, &failed, d_nfail, 1));
    // ---- second pass: A over the subjects that did not fail, and the quadratic forms (they need b and d complete).  One
    // chunk: its rows are still there.  Several: the launches run again -- for the quadratic forms always, for A only where
    // a subject failed, which the host has to ask the device about
    bool again = want_q || (want_a && single);
    if (a_along) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        again = failed > 0;
    }
    if (again) {
        for (int l0 = 0; l0 < n_live; l0 += (int)chunk) {
            const int kn = (int)std::min<int64_t>(chunk, n_live - l0);
            if (!single && (rc = solve(l0, kn))) return rc;
            if (want_a) HIP_TRY(cude::launch_info_cross(ia, kn, l0, l0 == 0, c->sc_rows.p, ia.status, d_part, c->stream));
            if (want_q) HIP_TRY(cude::launch_info_qform(ia, kn, l0, profiled != 0, c->sc_rows.p, d_gcond, d_cov, c->stream));
        }
    }
    if (want_a) HIP_TRY(cude::launch_info_cross_finish(ia, d_part, d_gn, c->stream));
    if (rq.want_schur) {
        HIP_TRY(cude::launch_info_cross(ia, 1, -1, true, ia.t, ia.status, d_partx, c->stream));
        HIP_TRY(cude::launch_info_cross_finish(ia, d_partx, d_x, c->stream));
        HIP_TRY(cude::launch_info_schur(P, d_gn, d_x, d_schur, c->stream));
    }
    tb.gn = d_gn; tb.schur = d_schur; tb.coup = d_coup; tb.nfail = d_nfail;
    return CUDE_OK;
}

extern "C" {

int32_t cude_simulate(cude_ctx* c, int32_t n_times, const double* times, double* traj) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if (!c->have_pop) return fail(CUDE_ERR_STATE, "population not set");
    if (!c->have_nn || !c->have_cond) return fail(CUDE_ERR_STATE, "parameters not set");
    if (n_times < 1 || !times || !traj) return fail(CUDE_ERR_ARG, "null/empty input");
    const bool cpep = is_cpep(c);
    const int NS = cpep ? c->cfg.n_state : 3;
    if ((rc = check_output_times(c, n_times, times))) return rc;
    const int64_t N = c->N;
    // output times per launch: ~1 GB of trajectory scratch at most (every launch integrates from t_0 again)
    const int64_t chunk = sets_per_launch(n_times, kNoGridCap, 1e9, 8.0 * NS * (double)N, c->opt.dense_chunk);
    // suppression model: the kernels write the caller's [3 x T x N] directly (8-byte stores 24 T bytes apart between the
    // lanes of a wave; L2 merges a lane's consecutive outputs) or, option "dense_layout" = 1, lane-contiguous rows
    // [T][3][N] (one 512-byte store per state, output time and wave) that a transpose kernel reorders.  Measured at 1e5
    // subjects, 301 times, 4-3x5-1 (cude_forward at the 8 data times: 0.40 / 0.41 ms): direct 0.56-0.72 ms (fixed step) /
    // 0.80-0.82 ms (adaptive) against rows 0.54-0.68 + 0.41-0.45 ms transpose / 1.13-1.15 + 0.41-0.46 ms -- the direct
    // stores are not the bottleneck, so they are the default.  The call itself (~365 ms) is host-side copying.
    const bool rows = !cpep && c->opt.dense_layout == 1;
    DevBuf<double> d_traj, d_rows;
    OutputTables tables;
    HIP_TRY(d_traj.resize((size_t)NS * chunk * N));
    if (rows) HIP_TRY(d_rows.resize((size_t)NS * chunk * N));
    if ((rc = tables.upload(c, n_times, times))) return rc;
    DenseLaunch d;
    d.cond = c->cond.p; d.partials = c->partials.p;
    d.traj = rows ? d_rows.p : d_traj.p;                    // what the solve writes
    for (int64_t k0 = 0; k0 < n_times; k0 += chunk) {
        const int64_t kn = std::min<int64_t>(chunk, n_times - k0);
        // outputs a failed adaptive solve does not reach stay NaN
        if (adaptive(c)) HIP_TRY(hipMemsetAsync(d.traj, 0xff, (size_t)NS * kn * N * sizeof(double), c->stream));
        d.k0 = k0; d.kn = kn;
        if (rows) { d.traj_ss = N; d.traj_st = 3 * N; d.traj_sn = 1; }
        else { d.traj_ss = 1; d.traj_st = 3; d.traj_sn = 3 * kn; }
        if ((rc = launch_dense(c, tables, d))) return rc;
        if (rows) HIP_TRY(cude::launch_supp_traj_transpose(N, (int)kn, d_rows.p, d_traj.p, c->stream));
        // device chunk [NS x kn x N] -> rows k0..k0+kn of the caller's [NS x n_times x N]
        HIP_TRY(hipMemcpy2DAsync(traj + (size_t)NS * k0, (size_t)NS * n_times * sizeof(double), d_traj.p,
                                 (size_t)NS * kn * sizeof(double), (size_t)NS * kn * sizeof(double), (size_t)N,
                                 hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));           // d_traj is the next chunk's too
    }
    return CUDE_OK;
}

int32_t cude_predictive_bands(cude_ctx* c, int32_t n_sets, const double* cond_sets, int32_t n_times, const double* times,
                              int32_t state, int32_t n_ranks, const int32_t* ranks, double* order_out, double* mean_out,
                              int32_t* bad_sets_out) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if (!c->have_pop) return fail(CUDE_ERR_STATE, "population not set");
    if (!c->have_nn) return fail(CUDE_ERR_STATE, "shared parameters not set");
    if (c->net.generic())
        return fail(CUDE_ERR_UNSUPPORTED, "cude_predictive_bands: the network of this context runs on the fallback kernel "
                                          "(cude_set_network), whose dense output takes one parameter set");
    if (c->capturing) return fail(CUDE_ERR_STATE, "cude_predictive_bands under stream capture");
    if (n_sets < 1 || n_sets > cude::kPredMaxSets) return fail(CUDE_ERR_ARG, "need 1 <= n_sets <= 4096");
    if (n_ranks < 0 || n_ranks > cude::kPredMaxRanks) return fail(CUDE_ERR_ARG, "need 0 <= n_ranks <= 16");
    if (!cond_sets || n_times < 1 || !times) return fail(CUDE_ERR_ARG, "null/empty input");
    if ((n_ranks > 0 && (!ranks || !order_out)) || (n_ranks == 0 && order_out) || (!order_out && !mean_out))
        return fail(CUDE_ERR_ARG, "need order_out with n_ranks > 0 ranks, or mean_out, or both");
    if (!ranks_increasing(n_ranks, ranks, n_sets)) return fail(CUDE_ERR_ARG, "ranks must be strictly increasing inside [0, n_sets)");
    const bool cpep = is_cpep(c);
    const int NS = cpep ? c->cfg.n_state : 3;
    if (state < 0 || state >= NS) return fail(CUDE_ERR_ARG, "state out of range");
    if ((rc = check_output_times(c, n_times, times))) return rc;
    const int64_t N = c->N, K = n_sets, nb = c->nblocks;
    const int P = c->P;
    // The sample trajectories of one launch: [K][subjects][Tc][NS], ~1 GB at most.  Whole workgroups of subjects first (no
    // solve is repeated); output times only when 64 subjects alone exceed the budget (each time chunk integrates from t_0)
    const double budget = 1e9, per_time = 8.0 * NS * (double)K * cude::kBlock;     // bytes of one output time of one workgroup
    int64_t Tc = n_times;
    if (c->opt.predictive_times > 0) Tc = std::min<int64_t>(n_times, c->opt.predictive_times);
    else if (per_time * n_times > budget) Tc = std::max<int64_t>(1, (int64_t)(budget / per_time));
    const SubjectPasses passes = subject_passes(N, nb, cude::kBlock, budget, per_time * (double)Tc, c->opt.predictive_subjects);
    DevBuf<double> d_cond, d_slab, d_part, d_order, d_mean;
    DevBuf<int32_t> d_ranks, d_count;
    OutputTables tables;
    DevBuf<uint8_t> d_bad;
    HIP_TRY(d_cond.resize((size_t)K * N));
    HIP_TRY(d_slab.resize((size_t)K * passes.sub_max * Tc * NS));
    if (cpep || adaptive(c)) HIP_TRY(d_part.resize((size_t)K * passes.blocks * (P + 2)));
    HIP_TRY(d_bad.resize((size_t)K * N));
    HIP_TRY(d_count.resize((size_t)N));
    if (n_ranks > 0) {
        HIP_TRY(d_ranks.resize((size_t)n_ranks));
        HIP_TRY(d_order.resize((size_t)n_ranks * n_times * N));
        HIP_TRY(push(c, d_ranks.p, ranks, n_ranks));
    }
    if (mean_out) HIP_TRY(d_mean.resize((size_t)n_times * N));
    HIP_TRY(push(c, d_cond.p, cond_sets, K * N));
    HIP_TRY(hipMemsetAsync(d_bad.p, 0, (size_t)K * N, c->stream));
    if ((rc = tables.upload(c, n_times, times))) return rc;
    DenseLaunch d;                                        // K sets; the caller's order of subjects
    d.cond = d_cond.p; d.n_sets = (int32_t)K; d.partials = d_part.p; d.keep_perm = false;
    d.traj_ss = 1; d.traj_st = 3;
    for (int64_t b = 0; b < nb; b += passes.blocks) {
        const auto [b0, bn, s0, sn] = passes.at(b);
        for (int64_t k0 = 0; k0 < n_times; k0 += Tc) {
            const int64_t kn = std::min<int64_t>(Tc, n_times - k0);
            const int64_t set_stride = (int64_t)NS * kn * sn;
            // outputs a failed adaptive solve does not reach stay NaN
            if (adaptive(c)) HIP_TRY(hipMemsetAsync(d_slab.p, 0xff, (size_t)K * set_stride * sizeof(double), c->stream));
            // subject i of the population writes column block (i - s0) of the slab
            d.traj = d_slab.p - (int64_t)NS * kn * s0;
            d.k0 = k0; d.kn = kn; d.traj_sn = 3 * kn;
            d.set_stride = set_stride; d.blk_first = b0; d.blk_count = bn;
            if ((rc = launch_dense(c, tables, d))) return rc;
            cude::PredictiveArgs pa{};
            pa.slab = d_slab.p + state; pa.set_stride = set_stride; pa.col_stride = NS; pa.n_cols = kn * sn;
            pa.K = (int32_t)K; pa.Tc = (int32_t)kn; pa.n_ranks = n_ranks;
            pa.subj0 = s0; pa.t0 = (int32_t)k0; pa.n_times = n_times;
            pa.order = d_order.p; pa.mean = d_mean.p;
            pa.bad = d_bad.p; pa.bad_stride = K;
            HIP_TRY(cude::launch_predictive_select(pa, d_ranks.p, c->stream));
        }
    }
    HIP_TRY(cude::launch_predictive_count(N, (int)K, d_bad.p, d_count.p, c->stream));
    std::vector<int32_t> count((size_t)N);
    HIP_TRY(fetch(c, count.data(), d_count.p, N));
    HIP_TRY(fetch(c, order_out, d_order.p, (size_t)n_ranks * n_times * N));
    HIP_TRY(fetch(c, mean_out, d_mean.p, (size_t)n_times * N));
    HIP_TRY(hipStreamSynchronize(c->stream));
    int64_t failed = 0;
    for (int64_t i = 0; i < N; i++) failed += count[(size_t)i] > 0;
    c->last_failed = failed;
    if (bad_sets_out) std::memcpy(bad_sets_out, count.data(), (size_t)N * sizeof(int32_t));
    return CUDE_OK;
}

int32_t cude_evaluate_conditional_sets(cude_ctx* c, int32_t n_sets, const double* cond_sets, double penalty_weight,
                                       double penalty_center, double* sse_out, int32_t* best_index_out,
                                       double* best_objective_out) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if (!c->have_pop) return fail(CUDE_ERR_STATE, "population not set");
    if (!c->have_nn) return fail(CUDE_ERR_STATE, "shared parameters not set");
    if (c->capturing) return fail(CUDE_ERR_STATE, "cude_evaluate_conditional_sets under stream capture");
    if (n_sets < 1 || !cond_sets) return fail(CUDE_ERR_ARG, "null/empty input");
    if (!sse_out && !best_index_out && !best_objective_out) return fail(CUDE_ERR_ARG, "no output requested");
    if (!(penalty_weight >= 0) || !std::isfinite(penalty_weight) || !std::isfinite(penalty_center))
        return fail(CUDE_ERR_ARG, "need a finite penalty_weight >= 0 and a finite penalty_center");
    const int64_t N = c->N;
    const int64_t chunk = profile_chunk_sets(c, n_sets);
    DevBuf<double> d_cond, d_sse, d_part, d_fmin;
    DevBuf<int32_t> d_imin;
    HIP_TRY(d_cond.resize((size_t)chunk * N));
    HIP_TRY(d_sse.resize((size_t)chunk * N));
    HIP_TRY(d_fmin.resize((size_t)N));
    HIP_TRY(d_imin.resize((size_t)N));
    if ((rc = reserve_sets_forward(c, chunk, false, d_part))) return rc;
    SetsForward fwd;                                      // one network, kn sets of per-subject values
    fwd.cond = d_cond.p; fwd.nn = c->nn.p; fwd.sse = d_sse.p; fwd.partials = d_part.p;
    for (int64_t k0 = 0; k0 < n_sets; k0 += chunk) {
        const int64_t kn = std::min<int64_t>(chunk, n_sets - k0);
        HIP_TRY(push(c, d_cond.p, cond_sets + k0 * N, kn * N));
        fwd.n_sets = (int)kn;
        if ((rc = forward_sets(c, fwd))) return rc;
        HIP_TRY(cude::launch_best_of_sets(N, (int)k0, (int)kn, d_sse.p, d_cond.p, penalty_weight, penalty_center, d_fmin.p,
                                          d_imin.p, c->stream));
        if (sse_out)
            HIP_TRY(fetch(c, sse_out + k0 * N, d_sse.p, kn * N));
        // (d_cond / d_sse are the next chunk's too; copies from and to pageable memory are staged by the runtime in
        //  stream order, so only the last chunk needs the host to wait)
    }
    HIP_TRY(fetch(c, best_index_out, d_imin.p, N));
    HIP_TRY(fetch(c, best_objective_out, d_fmin.p, N));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CUDE_OK;
}

int32_t cude_marginal_likelihood(cude_ctx* c, int32_t n_nodes, const double* nodes, const double* log_weights,
                                 int64_t first_step, const double* center, const double* scale, double sigma,
                                 double prior_mean, double prior_sd, double* logml_out, double* post_mean_out,
                                 double* post_var_out, double* post_sse_out, double* ess_out, int32_t* n_bad_out,
                                 double* points_out, double* terms_out) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if (!c->have_pop) return fail(CUDE_ERR_STATE, "population not set");
    if (!c->have_nn) return fail(CUDE_ERR_STATE, "shared parameters not set");
    if (!center && !c->have_cond) return fail(CUDE_ERR_STATE, "center is NULL and the conditional parameters are not set");
    if (c->capturing) return fail(CUDE_ERR_STATE, "cude_marginal_likelihood under stream capture");
    if (n_nodes < 1 || n_nodes > 65536) return fail(CUDE_ERR_ARG, "n_nodes must lie in 1 ... 65536");
    if ((nodes == nullptr) != (log_weights == nullptr)) return fail(CUDE_ERR_ARG, "pass both nodes and log_weights or neither");
    const bool draws = nodes == nullptr;
    if (!draws) {
        for (int32_t k = 0; k < n_nodes; k++)
            if (!std::isfinite(nodes[k]) || !std::isfinite(log_weights[k]))
                return fail(CUDE_ERR_ARG, "nodes and log_weights must be finite");
    }
    if (first_step < 0) return fail(CUDE_ERR_ARG, "first_step must be >= 0");
    if (!(sigma > 0) || !std::isfinite(sigma)) return fail(CUDE_ERR_ARG, "sigma must be finite and > 0");
    if (!(prior_sd > 0)) return fail(CUDE_ERR_ARG, "prior_sd must be > 0 (+Inf: no prior term)");
    if (!std::isfinite(prior_mean)) return fail(CUDE_ERR_ARG, "prior_mean must be finite");
    if (!logml_out && !post_mean_out && !post_var_out && !post_sse_out && !ess_out && !n_bad_out && !points_out && !terms_out)
        return fail(CUDE_ERR_ARG, "no output requested");
    const int64_t N = c->N;
    const int64_t chunk = profile_chunk_sets(c, n_nodes);
    DevBuf<double> d_x, d_z, d_sse, d_terms, d_part, d_rule, d_in, d_state, d_out;
    DevBuf<int32_t> d_bad;              // [N] bad nodes, then the number of subjects without a finite term
    HIP_TRY(d_x.resize((size_t)chunk * N));
    HIP_TRY(d_sse.resize((size_t)chunk * N));
    if (draws) HIP_TRY(d_z.resize((size_t)chunk * N));
    if (terms_out) HIP_TRY(d_terms.resize((size_t)chunk * N));
    HIP_TRY(d_state.resize((size_t)cude::kMarginalState * N));
    HIP_TRY(d_out.resize((size_t)5 * N));
    HIP_TRY(d_bad.resize((size_t)N + 1));
    if ((rc = reserve_sets_forward(c, chunk, false, d_part))) return rc;
    cude::MarginalArgs m{};
    m.N = N; m.n_nodes = n_nodes;
    if (!draws) {
        HIP_TRY(d_rule.resize((size_t)2 * n_nodes));
        HIP_TRY(push(c, d_rule.p, nodes, n_nodes));
        HIP_TRY(push(c, d_rule.p + n_nodes, log_weights, n_nodes));
        m.nodes = d_rule.p; m.log_weights = d_rule.p + n_nodes;
    }
    if (center || scale) HIP_TRY(d_in.resize((size_t)2 * N));
    m.center = c->cond.p;
    if (center) {
        HIP_TRY(push(c, d_in.p, center, N));
        m.center = d_in.p;
    }
    if (scale) {
        HIP_TRY(push(c, d_in.p + N, scale, N));
        m.scale = d_in.p + N;
    }
    // the stream's key at first_step; the context's own position (rng_step) is neither read nor advanced
    m.key = cude::RngKey{c->rng_seed, c->rng_offset, first_step};
    m.c_K = 0.91893853320467274178 - std::log((double)n_nodes);   // 0.5 log(2 pi) - log K
    m.ll_const = -(c->T / 2.0) * std::log(sigma * sigma);        // cude_mh_chain's
    m.inv_2s2 = 1.0 / (2.0 * sigma * sigma);
    m.prior_mean = prior_mean; m.prior_sd = prior_sd;
    m.log_prior_sd = std::isfinite(prior_sd) ? std::log(prior_sd) : 0.0;
    m.state = d_state.p; m.n_bad = d_bad.p;
    SetsForward fwd;                                      // one network, kn sets of per-subject values
    fwd.cond = d_x.p; fwd.nn = c->nn.p; fwd.sse = d_sse.p; fwd.partials = d_part.p;
    for (int64_t k0 = 0; k0 < n_nodes; k0 += chunk) {
        const int64_t kn = std::min<int64_t>(chunk, n_nodes - k0);
        HIP_TRY(cude::launch_marginal_points(m, (int)k0, (int)kn, d_x.p, d_z.p, c->stream));
        fwd.n_sets = (int)kn;
        if ((rc = forward_sets(c, fwd))) return rc;
        HIP_TRY(cude::launch_marginal_accumulate(m, (int)k0, (int)kn, d_sse.p, d_x.p, d_z.p, d_terms.p, c->stream));
        if (points_out)
            HIP_TRY(fetch(c, points_out + k0 * N, d_x.p, kn * N));
        if (terms_out)
            HIP_TRY(fetch(c, terms_out + k0 * N, d_terms.p, kn * N));
        // (the chunk buffers are the next chunk's too: copies to pageable memory are staged in stream order)
    }
    HIP_TRY(hipMemsetAsync(d_bad.p + N, 0, sizeof(int32_t), c->stream));
    double* const o = d_out.p;
    HIP_TRY(cude::launch_marginal_finish(m, o, o + N, o + 2 * N, o + 3 * N, o + 4 * N, d_bad.p + N, c->stream));
    double* const outs[5] = {logml_out, post_mean_out, post_var_out, post_sse_out, ess_out};
    for (int q = 0; q < 5; q++)
        HIP_TRY(fetch(c, outs[q], o + (size_t)q * N, N));
    HIP_TRY(fetch(c, n_bad_out, d_bad.p, N));
    int32_t failed = 0;
    HIP_TRY(fetch(c, &failed, d_bad.p + N, 1));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->last_failed = failed;
    return CUDE_OK;
}

int32_t cude_subject_scores(cude_ctx* c, int32_t n_sets, const double* cond_sets, const double* weights, double* score_out,
                            double* wsse_out, int32_t* bad_out, double* sum_out, double* cross_out) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if (!c->have_pop) return fail(CUDE_ERR_STATE, "population not set");
    if (!c->have_nn) return fail(CUDE_ERR_STATE, "shared parameters not set");
    if (c->capturing) return fail(CUDE_ERR_STATE, "cude_subject_scores under stream capture");
    if (n_sets < 1) return fail(CUDE_ERR_ARG, "n_sets must be >= 1");
    if (!cond_sets && n_sets > 1) return fail(CUDE_ERR_ARG, "cond_sets is NULL with n_sets > 1");
    if (!cond_sets && !c->have_cond) return fail(CUDE_ERR_STATE, "cond_sets is NULL and the conditional parameters are not set");
    if (!score_out && !wsse_out && !bad_out && !sum_out && !cross_out) return fail(CUDE_ERR_ARG, "no output requested");
    const int P = c->P;
    const int64_t N = c->N, K = n_sets;
    if (weights)
        for (int64_t j = 0; j < K * N; j++)
            if (!std::isfinite(weights[j])) return fail(CUDE_ERR_ARG, "weights must be finite");
    const int64_t chunk = scores_chunk_sets(c, K);
    // per-set rows: conditionals, weights, SSEs, conditional gradients (scratch of the launch)
    HIP_TRY(c->sc_rows.reserve((size_t)chunk * P * N));
    HIP_TRY(c->sc_sets.reserve((size_t)chunk * 4 * N));
    HIP_TRY(c->ms_out.reserve((size_t)chunk * (P + 2)));
    double* const d_cond = c->sc_sets.p;
    double* const d_w = d_cond + chunk * N;
    double* const d_sse = d_w + chunk * N;
    double* const d_gcond = d_sse + chunk * N;
    cude::ScoresArgs sa{};
    sa.N = N; sa.P = P;
    // state (the kernels take wsse at s + P N and fail at bad + N)
    double *d_table = nullptr, *d_sum = nullptr, *d_cross = nullptr;
    int32_t* d_nfail = nullptr;
    HIP_TRY(carve(c->sc_state, [&](Carve<double>& v) {
        sa.s = v.take((size_t)P * N);           // [P][N]
        sa.wsse = v.take(N);
        d_table = v.take((size_t)P * N);        // the caller's [N][P] table
        d_sum = v.take(P);
        d_cross = v.take((size_t)P * P);
    }));
    HIP_TRY(carve(c->sc_int, [&](Carve<int32_t>& v) {
        sa.bad = v.take(N);
        sa.fail = v.take(N);
        d_nfail = v.take(1);
    }));
    const SetsRows rows{c->sc_rows.p, d_sse};
    for (int64_t k0 = 0; k0 < K; k0 += chunk) {
        const int64_t kn = std::min<int64_t>(chunk, K - k0);
        const double* cond_k = c->cond.p;                         // (NULL: the context's own conditionals, one set)
        if (cond_sets) {
            HIP_TRY(push(c, d_cond, cond_sets + k0 * N, kn * N));
            cond_k = d_cond;
        }
        if (weights)
            HIP_TRY(push(c, d_w, weights + k0 * N, kn * N));
        if ((rc = eval_sets_device(c, kn, c->nn.p, 0, cond_k, N, d_gcond, c->ms_out.p, &rows))) return rc;
        HIP_TRY(cude::launch_scores_fold(sa, (int)kn, k0 == 0, c->sc_rows.p, d_sse, weights ? d_w : nullptr, c->stream));
        // (the chunk buffers are the next chunk's too: copies from pageable memory are staged in stream order)
    }
    HIP_TRY(hipMemsetAsync(d_nfail, 0, sizeof(int32_t), c->stream));
    HIP_TRY(cude::launch_scores_finish(sa, c->param_mask.p, d_nfail, score_out ? d_table : nullptr, c->stream));
    if (sum_out || cross_out) {
        HIP_TRY(c->sc_part.reserve(cude::scores_cross_partials(N, P)));
        HIP_TRY(cude::launch_scores_cross(sa, c->sc_part.p, d_sum, d_cross, c->stream));
    }
    HIP_TRY(fetch(c, score_out, d_table, (size_t)P * N));
    HIP_TRY(fetch(c, wsse_out, sa.wsse, N));
    HIP_TRY(fetch(c, bad_out, sa.bad, N));
    HIP_TRY(fetch(c, sum_out, d_sum, P));
    HIP_TRY(fetch(c, cross_out, d_cross, (size_t)P * P));
    int32_t failed = 0;
    HIP_TRY(fetch(c, &failed, d_nfail, 1));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->last_failed = failed;
    return CUDE_OK;
}

int32_t cude_network_information(cude_ctx* c, const double* cond, double penalty_weight, const double* cov, int32_t profiled,
                                 double* jac_out, double* jcond_out, double* gn_out, double* coupling_out, double* dcond_out,
                                 double* schur_out, double* qform_out, int32_t* status_out) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if (!c->have_pop) return fail(CUDE_ERR_STATE, "population not set");
    if (!c->have_nn) return fail(CUDE_ERR_STATE, "shared parameters not set");
    if (!cond && !c->have_cond) return fail(CUDE_ERR_STATE, "cond is NULL and the conditional parameters are not set");
    if (c->capturing) return fail(CUDE_ERR_STATE, "cude_network_information under stream capture");
    if (!jac_out && !jcond_out && !gn_out && !coupling_out && !dcond_out && !schur_out && !qform_out && !status_out)
        return fail(CUDE_ERR_ARG, "no output requested");
    if (qform_out && !cov) return fail(CUDE_ERR_ARG, "qform_out needs cov");
    if (!(penalty_weight >= 0.0) || !std::isfinite(penalty_weight))
        return fail(CUDE_ERR_ARG, "penalty_weight must be finite and >= 0");
    const int P = c->P;
    const int64_t N = c->N;
    if (cov && qform_out)
        for (int64_t j = 0; j < (int64_t)P * P; j++)
            if (!std::isfinite(cov[j])) return fail(CUDE_ERR_ARG, "cov must be finite");
    InfoRequest rq;
    rq.cond = cond; rq.pw = penalty_weight; rq.cov = cov; rq.profiled = profiled != 0; rq.jac_out = jac_out;
    rq.want_a = gn_out || schur_out; rq.want_schur = schur_out != nullptr; rq.want_q = qform_out != nullptr;
    InfoTables tb;
    if ((rc = info_pass(c, rq, tb))) return rc;
    const cude::InfoArgs& ia = tb.ia;
    const int n_out = ia.n_out;
    double *const d_coup = tb.coup, *const d_gn = tb.gn, *const d_schur = tb.schur;
    int32_t& failed = tb.failed;
    if (coupling_out) {
        HIP_TRY(cude::launch_info_transpose(ia, 1, -1, 1, ia.b, false, d_coup, c->stream));
        HIP_TRY(fetch(c, coupling_out, d_coup, (size_t)P * N));
    }
    HIP_TRY(fetch(c, jcond_out, ia.jc, (size_t)n_out * N));
    HIP_TRY(fetch(c, qform_out, ia.qf, (size_t)n_out * N));
    HIP_TRY(fetch(c, dcond_out, ia.d, N));
    HIP_TRY(fetch(c, gn_out, d_gn, (size_t)P * P));
    HIP_TRY(fetch(c, schur_out, d_schur, (size_t)P * P));
    std::vector<int32_t> st_host;
    std::vector<double> mask_host;
    int32_t* st = status_out;
    if (jac_out && !st) { st_host.resize((size_t)N); st = st_host.data(); }
    HIP_TRY(fetch(c, st, ia.status, N));
    if (jac_out && ia.mask) {
        mask_host.resize((size_t)P);
        HIP_TRY(fetch(c, mask_host.data(), ia.mask, P));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->last_failed = failed;
    // (a failure shows only once every output is in, and the Jacobian's chunks have left the device by then)
    if (jac_out && failed > 0) {
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (int64_t i = 0; i < N; i++) {
            if (!(st[i] & 1)) continue;
            double* row = jac_out + (size_t)i * n_out * P;
            for (int o = 0; o < n_out; o++)
                for (int q = 0; q < P; q++) row[(size_t)o * P + q] = (!mask_host.empty() && mask_host[q] == 0.0) ? 0.0 : nan;
        }
    }
    return CUDE_OK;
}

int32_t cude_sensitivity(cude_ctx* c, double* sens, double* info, double* score, double* sse) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if (!c->have_pop) return fail(CUDE_ERR_STATE, "population not set");
    if (!c->have_nn || !c->have_cond) return fail(CUDE_ERR_STATE, "parameters not set");
    if (c->net.generic())
        return fail(CUDE_ERR_UNSUPPORTED, "cude_sensitivity: the network of this context runs on the fallback kernel "
                                          "(cude_set_network), which has no tangent-linear solve");
    if (c->capturing) return fail(CUDE_ERR_STATE, "cude_sensitivity under stream capture");
    const bool cpep = is_cpep(c);
    const int NS = cpep ? c->cfg.n_state : 3;
    const int64_t N = c->N;
    if (sens) HIP_TRY(c->sens.reserve((size_t)NS * c->T * N));
    HIP_TRY(c->sens_info.reserve((size_t)N));
    HIP_TRY(c->sens_score.reserve((size_t)N));
    // adaptive mode: the accepted steps go to the gradient's tape, so that cude_adaptive_steps reports them
    if (adaptive(c) && (rc = ensure_tape(c))) return rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (c->timing && (c->timing_count++ % c->timing_period) == 0 && (rc = timed_pair(c, &e0, &e1))) return rc;
    cude::SensOut out;
    out.sens = sens ? c->sens.p : nullptr;
    out.info = c->sens_info.p;
    out.score = c->sens_score.p;
    const hipError_t le = launch_tangent(c, c->cond.p, c->sse.p, out, true);
    if (le == hipErrorInvalidValue) return fail(CUDE_ERR_UNSUPPORTED, "cude_sensitivity: no tangent kernel compiled for this network shape / model");
    HIP_TRY(le);
    if (e1) HIP_TRY(hipEventRecord(e1, c->stream));
    note_adaptive_launch(c, true);
    // [sum SSE, n_failed] behind the launch, as a forward evaluation's (finish_loss sets cude_n_failed)
    c->loss_in_pinned = false;
    c->tail_in_pinned = false;
    HIP_TRY(cude::launch_reduce_cols(c->partials.p, c->nblocks, c->P + 2, c->P, 2, c->g_nn.p, c->stream));
    HIP_TRY(fetch(c, sens, c->sens.p, (size_t)NS * c->T * N));
    HIP_TRY(fetch(c, info, c->sens_info.p, N));
    HIP_TRY(fetch(c, score, c->sens_score.p, N));
    HIP_TRY(fetch(c, sse, c->sse.p, N));
    return finish_loss(c, nullptr, nullptr);
}

int32_t cude_curvature(cude_ctx* c, double* sens2, double* curv, double* info, double* score, double* sse) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if (!c->have_pop) return fail(CUDE_ERR_STATE, "population not set");
    if (!c->have_nn || !c->have_cond) return fail(CUDE_ERR_STATE, "parameters not set");
    if (c->net.generic())
        return fail(CUDE_ERR_UNSUPPORTED, "cude_curvature: the network of this context runs on the fallback kernel "
                                          "(cude_set_network), which has no forward-mode solve");
    if (c->capturing) return fail(CUDE_ERR_STATE, "cude_curvature under stream capture");
    if (!sens2 && !curv && !info && !score && !sse) return fail(CUDE_ERR_ARG, "cude_curvature: no output requested");
    const bool cpep = is_cpep(c);
    const int NS = cpep ? c->cfg.n_state : 3;
    const int64_t N = c->N;
    if (sens2) HIP_TRY(c->sens2.reserve((size_t)NS * c->T * N));
    HIP_TRY(c->sens_curv.reserve((size_t)N));
    HIP_TRY(c->sens_info.reserve((size_t)N));
    HIP_TRY(c->sens_score.reserve((size_t)N));
    // adaptive mode: the accepted steps go to the gradient's tape, so that cude_adaptive_steps reports them
    if (adaptive(c) && (rc = ensure_tape(c))) return rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (c->timing && (c->timing_count++ % c->timing_period) == 0 && (rc = timed_pair(c, &e0, &e1))) return rc;
    cude::SensOut out;
    out.info = c->sens_info.p;
    out.score = c->sens_score.p;
    cude::CurvOut out2;
    out2.sens2 = sens2 ? c->sens2.p : nullptr;
    out2.curv = c->sens_curv.p;
    const hipError_t le = launch_tangent2(c, c->cond.p, c->sse.p, out, out2, true);
    if (le == hipErrorInvalidValue) return fail(CUDE_ERR_UNSUPPORTED, "cude_curvature: no order-2 kernel compiled for this network shape / model");
    HIP_TRY(le);
    if (e1) HIP_TRY(hipEventRecord(e1, c->stream));
    note_adaptive_launch(c, true);
    // [sum SSE, n_failed] behind the launch, as cude_sensitivity
    c->loss_in_pinned = false;
    c->tail_in_pinned = false;
    HIP_TRY(cude::launch_reduce_cols(c->partials.p, c->nblocks, c->P + 2, c->P, 2, c->g_nn.p, c->stream));
    HIP_TRY(fetch(c, sens2, c->sens2.p, (size_t)NS * c->T * N));
    HIP_TRY(fetch(c, curv, c->sens_curv.p, N));
    HIP_TRY(fetch(c, info, c->sens_info.p, N));
    HIP_TRY(fetch(c, score, c->sens_score.p, N));
    HIP_TRY(fetch(c, sse, c->sse.p, N));
    return finish_loss(c, nullptr, nullptr);
}

int32_t cude_multistart_forward(cude_ctx* c, int32_t n_sets, const double* nn_sets, const double* cond_sets,
                                double* losses) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if (!c->have_pop) return fail(CUDE_ERR_STATE, "population not set");
    if (n_sets < 1 || !nn_sets || !cond_sets || !losses) return fail(CUDE_ERR_ARG, "null/empty input");
    const int P = c->P;
    const int64_t N = c->N, nb = c->nblocks;
    // chunk so that one launch stays below 2^16-1 grid rows and ~256 MB of partials
    const int64_t chunk = sets_per_launch(n_sets, 32768, 256e6, (double)nb * (P + 2) * 8.0);
    DevBuf<double> d_nn, d_cond, d_part, d_out;
    HIP_TRY(d_nn.resize((size_t)chunk * P));
    HIP_TRY(d_cond.resize((size_t)chunk * N));
    if ((rc = reserve_sets_forward(c, chunk, false, d_part))) return rc;
    HIP_TRY(d_out.resize((size_t)chunk * 2));
    std::vector<double> h_out((size_t)chunk * 2);
    double reg = 0.0;
    SetsForward fwd;                                      // (network, conditional parameters) pairs
    fwd.cond = d_cond.p; fwd.nn = d_nn.p; fwd.stride_nn = P; fwd.partials = d_part.p;
    for (int64_t k0 = 0; k0 < n_sets; k0 += chunk) {
        const int64_t kn = std::min<int64_t>(chunk, n_sets - k0);
        HIP_TRY(push(c, d_nn.p, nn_sets + k0 * P, kn * P));
        HIP_TRY(push(c, d_cond.p, cond_sets + k0 * N, kn * N));
        fwd.n_sets = (int)kn;
        if ((rc = forward_sets(c, fwd))) return rc;
        HIP_TRY(cude::launch_reduce_sets(d_part.p, (int)kn, nb, P + 2, P, d_out.p, c->stream));
        if (distributed(c) && (rc = allreduce_dev(c, d_out.p, (size_t)kn * 2))) return rc;
        HIP_TRY(fetch(c, h_out.data(), d_out.p, kn * 2));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->xchg.ready && (rc = xchg_check(c))) return rc;
        for (int64_t k = 0; k < kn; k++) {
            reg = 0.0;
            if (c->cfg.lambda != 0.0) {
                const double* w = nn_sets + (k0 + k) * P;
                for (int q = 0; q < P; q++) reg += w[q] * w[q];
            }
            const double sum = h_out[2 * k], nf = h_out[2 * k + 1];
            losses[k0 + k] = (nf > 0.0 || !std::isfinite(sum)) ? std::numeric_limits<double>::infinity()
                                                             : sum / c->n_global + c->cfg.lambda * reg;
        }
    }
    return CUDE_OK;
}

int32_t cude_screen_candidates(cude_ctx* c, int64_t n_candidates, int32_t n_keep, cude_candidate_fn gen, void* user,
                               int64_t* index_out, double* loss_out, double* nn_out, double* cond_out) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if (!c->have_pop) return fail(CUDE_ERR_STATE, "population not set");
    if (n_candidates < 1 || n_keep < 1 || n_keep > 4096 || !gen || !index_out || !loss_out || !nn_out || !cond_out)
        return fail(CUDE_ERR_ARG, "bad argument (1 <= n_keep <= 4096)");
    if (n_keep > n_candidates) n_keep = (int32_t)n_candidates;
    const int P = c->P;
    const int64_t N = c->N, nb = c->nblocks;
    // candidates per launch: the grid's y dimension and ~256 MB of partial rows; the host holds ONE chunk at a time
    int64_t chunk = sets_per_launch(n_candidates, 32768, 256e6, (double)nb * (P + 2) * 8.0);
    chunk = sets_per_launch(chunk, 32768, 512e6, (double)(P + N) * 8.0);
    DevBuf<double> d_nn, d_cond, d_part, d_sums, d_loss, d_work, b_loss[2], b_nn[2], b_cond[2];
    DevBuf<long long> b_idx[2];
    DevBuf<int> d_sel;
    HIP_TRY(d_nn.resize((size_t)chunk * P));
    HIP_TRY(d_cond.resize((size_t)chunk * N));
    if ((rc = reserve_sets_forward(c, chunk, false, d_part))) return rc;
    HIP_TRY(d_sums.resize((size_t)chunk * 2));
    HIP_TRY(d_loss.resize((size_t)chunk));
    HIP_TRY(d_work.resize((size_t)chunk + n_keep));
    HIP_TRY(d_sel.resize((size_t)n_keep));
    for (int b = 0; b < 2; b++) {
        HIP_TRY(b_loss[b].resize(n_keep));
        HIP_TRY(b_idx[b].resize(n_keep));
        HIP_TRY(b_nn[b].resize((size_t)n_keep * P));
        HIP_TRY(b_cond[b].resize((size_t)n_keep * N));
    }
    std::vector<double> h_nn((size_t)chunk * P), h_cond((size_t)chunk * N);
    int have = 0, cur = 0;
    SetsForward fwd;                                      // (network, conditional parameters) pairs
    fwd.cond = d_cond.p; fwd.nn = d_nn.p; fwd.stride_nn = P; fwd.partials = d_part.p;
    for (int64_t k0 = 0; k0 < n_candidates; k0 += chunk) {
        const int64_t kn = std::min<int64_t>(chunk, n_candidates - k0);
        if (gen(k0, (int32_t)kn, h_nn.data(), h_cond.data(), user) < 0)
            return fail(CUDE_ERR_ARG, "candidate generator reported an error");
        HIP_TRY(push(c, d_nn.p, h_nn.data(), kn * P));
        HIP_TRY(push(c, d_cond.p, h_cond.data(), kn * N));
        fwd.n_sets = (int)kn;
        if ((rc = forward_sets(c, fwd))) return rc;
        HIP_TRY(cude::launch_reduce_sets(d_part.p, (int)kn, nb, P + 2, P, d_sums.p, c->stream));
        if (distributed(c) && (rc = allreduce_dev(c, d_sums.p, (size_t)kn * 2))) return rc;
        HIP_TRY(cude::launch_set_losses((int)kn, d_sums.p, d_nn.p, P, c->cfg.lambda, c->n_global, d_loss.p, c->stream));
        cude::TopkArgs t{};
        t.n_keep = n_keep; t.n_have = have; t.n_new = (int)kn; t.first = k0;
        t.best_loss = b_loss[cur].p; t.best_idx = b_idx[cur].p; t.chunk_loss = d_loss.p; t.work = d_work.p;
        t.new_loss = b_loss[1 - cur].p; t.new_idx = b_idx[1 - cur].p; t.sel_src = d_sel.p;
        HIP_TRY(cude::launch_topk_merge(t, P, N, b_nn[cur].p, b_cond[cur].p, d_nn.p, d_cond.p, b_nn[1 - cur].p,
                                        b_cond[1 - cur].p, c->stream));
        have = (int)std::min<int64_t>(n_keep, have + kn);
        cur = 1 - cur;
        HIP_TRY(hipStreamSynchronize(c->stream));            // the host chunk buffers are refilled by the next gen()
        if (c->xchg.ready && (rc = xchg_check(c))) return rc;
    }
    std::vector<long long> idx(n_keep);
    HIP_TRY(fetch(c, idx.data(), b_idx[cur].p, n_keep));
    HIP_TRY(fetch(c, loss_out, b_loss[cur].p, n_keep));
    HIP_TRY(fetch(c, nn_out, b_nn[cur].p, (size_t)n_keep * P));
    HIP_TRY(fetch(c, cond_out, b_cond[cur].p, (size_t)n_keep * N));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int r = 0; r < n_keep; r++) index_out[r] = idx[r];
    return CUDE_OK;
}

int32_t cude_multistart_loss_grad(cude_ctx* c, int32_t n_sets, const double* nn_sets, const double* cond_sets,
                                  double* losses, double* g_nn_sets, double* g_cond_sets) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if (!c->have_pop) return fail(CUDE_ERR_STATE, "population not set");
    if (n_sets < 1 || !nn_sets || !cond_sets || !losses || !g_nn_sets || !g_cond_sets)
        return fail(CUDE_ERR_ARG, "null/empty input");
    const int P = c->P;
    const int64_t N = c->N, K = n_sets;
    HIP_TRY(c->ms_nn.reserve((size_t)K * P));
    HIP_TRY(c->ms_cond.reserve((size_t)K * N));
    HIP_TRY(c->ms_gcond.reserve((size_t)K * N));
    HIP_TRY(c->ms_out.reserve((size_t)K * (P + 2)));
    HIP_TRY(c->ms_f.reserve((size_t)K));
    HIP_TRY(push(c, c->ms_nn.p, nn_sets, (size_t)K * P));
    HIP_TRY(push(c, c->ms_cond.p, cond_sets, (size_t)K * N));
    if ((rc = eval_sets_device(c, K, c->ms_nn.p, P, c->ms_cond.p, N, c->ms_gcond.p, c->ms_out.p))) return rc;
    // loss and L2 term per set, in the arithmetic of l2_term_kernel: a set's loss and gradient are bit-identical to
    // cude_loss_grad at the same parameters
    cude::FinishSetsArgs fa{};
    fa.P = P; fa.out = c->ms_out.p; fa.nn = c->ms_nn.p; fa.stride_nn = P; fa.lambda = c->cfg.lambda; fa.n_global = c->n_global;
    fa.mask = c->param_mask.p; fa.f = c->ms_f.p;
    HIP_TRY(cude::launch_finish_sets(fa, (int)K, c->stream));
    HIP_TRY(fetch(c, losses, c->ms_f.p, K));
    HIP_TRY(hipMemcpy2DAsync(g_nn_sets, (size_t)P * sizeof(double), c->ms_out.p, (size_t)(P + 2) * sizeof(double),
                             (size_t)P * sizeof(double), (size_t)K, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(fetch(c, g_cond_sets, c->ms_gcond.p, (size_t)K * N));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return c->xchg.ready ? xchg_check(c) : CUDE_OK;
}

int32_t cude_profile_conditional(cude_ctx* c, int32_t n_points, const double* values, double* sse_out) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if (!c->have_pop) return fail(CUDE_ERR_STATE, "population not set");
    if (!c->have_nn) return fail(CUDE_ERR_STATE, "shared parameters not set");
    if (n_points < 1 || !values || !sse_out) return fail(CUDE_ERR_ARG, "null/empty input");
    const int64_t N = c->N;
    const int64_t chunk = profile_chunk_sets(c, n_points);
    DevBuf<double> d_val, d_cond, d_sse, d_part;
    HIP_TRY(d_val.resize((size_t)chunk));
    HIP_TRY(d_cond.resize((size_t)chunk * N));
    HIP_TRY(d_sse.resize((size_t)chunk * N));
    if ((rc = reserve_sets_forward(c, chunk, false, d_part))) return rc;
    SetsForward fwd;                                      // one network, kn grid values
    fwd.cond = d_cond.p; fwd.nn = c->nn.p; fwd.sse = d_sse.p; fwd.partials = d_part.p;
    for (int64_t k0 = 0; k0 < n_points; k0 += chunk) {
        const int64_t kn = std::min<int64_t>(chunk, n_points - k0);
        HIP_TRY(push(c, d_val.p, values + k0, kn));
        HIP_TRY(cude::launch_fill_rows(N, (int)kn, d_val.p, d_cond.p, c->stream));
        fwd.n_sets = (int)kn;
        if ((rc = forward_sets(c, fwd))) return rc;
        HIP_TRY(fetch(c, sse_out + k0 * N, d_sse.p, kn * N));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return CUDE_OK;
}

int32_t cude_profile_intervals(cude_ctx* c, int32_t n_points, const double* values, const double* center, double delta,
                               const double* delta_per_subject, double penalty_weight, double penalty_center,
                               int32_t n_rounds, int32_t n_sections, double* lower_out, double* upper_out,
                               double* argmin_out, double* min_out, double* center_objective_out, int32_t* n_inside_out,
                               int32_t* status_out) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if (!c->have_pop) return fail(CUDE_ERR_STATE, "population not set");
    if (!c->have_nn) return fail(CUDE_ERR_STATE, "shared parameters not set");
    if (c->capturing) return fail(CUDE_ERR_STATE, "cude_profile_intervals under stream capture");
    if (n_points < 2 || !values) return fail(CUDE_ERR_ARG, "need n_points >= 2 and the scan values");
    for (int32_t k = 0; k < n_points; k++)
        if (!std::isfinite(values[k]) || (k > 0 && !(values[k] > values[k - 1])))
            return fail(CUDE_ERR_ARG, "the scan values must be finite and strictly increasing");
    if (n_rounds < 0 || n_rounds > 64 || n_sections < 1 || n_sections > cude::kProfileMaxSections)
        return fail(CUDE_ERR_ARG, "need 0 <= n_rounds <= 64 and 1 <= n_sections <= 16");
    if (!(penalty_weight >= 0) || !std::isfinite(penalty_weight) || !std::isfinite(penalty_center))
        return fail(CUDE_ERR_ARG, "need a finite penalty_weight >= 0 and a finite penalty_center");
    // rule 6: with the minimum and its place alone asked for there is no centre and no threshold
    const bool intervals = lower_out || upper_out || center_objective_out || n_inside_out || status_out;
    if (!intervals && !argmin_out && !min_out) return fail(CUDE_ERR_ARG, "no output requested");
    const int64_t N = c->N;
    if (intervals) {
        if (!center && !c->have_cond) return fail(CUDE_ERR_STATE, "no centre: conditional parameters not set and center is null");
        if (delta_per_subject) {
            for (int64_t i = 0; i < N; i++)
                if (!(delta_per_subject[i] >= 0)) return fail(CUDE_ERR_ARG, "delta_per_subject must be >= 0 (may be +Inf)");
        } else if (!(delta >= 0)) {
            return fail(CUDE_ERR_ARG, "delta must be >= 0 (may be +Inf)");
        }
    }
    const int m = n_sections, rounds = intervals ? n_rounds : 0;
    const int64_t chunk = profile_chunk_sets(c, n_points);
    const int64_t max_sets = std::max<int64_t>(chunk, rounds > 0 ? 2 * m : 1);
    const int rows = cude::profile_reduce_rows(N, (int)chunk);
    // device scratch: one chunk of conditional sets and SSEs, the reduction's partial rows and 9 + 5 numbers per subject
    DevBuf<double> d_val, d_cond, d_sse, d_part, d_state, d_pf;
    DevBuf<int32_t> d_istate, d_pi;
    HIP_TRY(d_val.resize((size_t)n_points));
    HIP_TRY(d_cond.resize((size_t)max_sets * N));
    HIP_TRY(d_sse.resize((size_t)max_sets * N));
    HIP_TRY(d_state.resize((size_t)11 * N));              // thr, fcen, fmin, lo_out, lo_in, hi_in, hi_out, argmin, centre, sse_c, delta
    HIP_TRY(d_istate.resize((size_t)5 * N));              // imin, first, last, cnt, status
    HIP_TRY(d_pf.resize((size_t)rows * N));
    HIP_TRY(d_pi.resize((size_t)4 * rows * N));
    if ((rc = reserve_sets_forward(c, max_sets, false, d_part))) return rc;
    double* q = d_state.p;
    cude::ProfileArgs a{};
    a.N = N; a.n_points = n_points; a.pw = penalty_weight; a.pc = penalty_center; a.values = d_val.p;
    a.thr = intervals ? q : nullptr; a.fcen = q + N; a.fmin = q + 2 * N;
    a.imin = d_istate.p; a.first = d_istate.p + N; a.last = d_istate.p + 2 * N; a.cnt = d_istate.p + 3 * N;
    a.p_fmin = d_pf.p;
    a.p_imin = d_pi.p; a.p_first = d_pi.p + (size_t)rows * N; a.p_last = d_pi.p + (size_t)2 * rows * N;
    a.p_cnt = d_pi.p + (size_t)3 * rows * N;
    cude::ProfileEnds e{};
    e.lo_out = q + 3 * N; e.lo_in = q + 4 * N; e.hi_in = q + 5 * N; e.hi_out = q + 6 * N; e.argmin = q + 7 * N;
    e.status = d_istate.p + 4 * N;
    double* d_center = q + 8 * N;
    double* d_sse_c = q + 9 * N;
    double* d_delta = q + 10 * N;
    HIP_TRY(push(c, d_val.p, values, n_points));
    const double* cen = nullptr;
    if (intervals) {                                      // rule 2: the centre, in one forward launch (cude_forward's own)
        cen = c->cond.p;
        if (center) {
            HIP_TRY(push(c, d_center, center, N));
            cen = d_center;
        }
        if (delta_per_subject)
            HIP_TRY(push(c, d_delta, delta_per_subject, N));
        if ((rc = run_ensemble(c, false, nullptr, true, cen, d_sse_c))) return rc;
    }
    HIP_TRY(cude::launch_profile_init(a, cen, d_sse_c, delta, delta_per_subject ? d_delta : nullptr, c->stream));
    SetsForward fwd;                                      // one network, kn grid values
    fwd.cond = d_cond.p; fwd.nn = c->nn.p; fwd.sse = d_sse.p; fwd.partials = d_part.p;
    for (int64_t k0 = 0; k0 < n_points; k0 += chunk) {    // rule 3: the scan, every chunk reduced where it is
        const int64_t kn = std::min<int64_t>(chunk, n_points - k0);
        HIP_TRY(cude::launch_fill_rows(N, (int)kn, d_val.p + k0, d_cond.p, c->stream));
        fwd.n_sets = (int)kn;
        if ((rc = forward_sets(c, fwd))) return rc;
        HIP_TRY(cude::launch_profile_reduce(a, (int)k0, (int)kn, d_sse.p, c->stream));
        if (k0 == 0 && (rc = maybe_regroup(c))) return rc; // (adaptive mode: the first launch has told the step counts)
    }
    HIP_TRY(cude::launch_profile_finish(a, e, c->stream));   // rule 4
    for (int r = 0; r < rounds; r++) {                    // rule 5: both ends of every subject, 2m sets per launch
        HIP_TRY(cude::launch_profile_round(a, e, m, 0, d_cond.p, d_sse.p, c->stream));
        fwd.n_sets = 2 * m;
        if ((rc = forward_sets(c, fwd))) return rc;
        HIP_TRY(cude::launch_profile_round(a, e, m, 1, d_cond.p, d_sse.p, c->stream));
    }
    std::vector<int32_t> status;
    HIP_TRY(fetch(c, lower_out, e.lo_in, N));
    HIP_TRY(fetch(c, upper_out, e.hi_in, N));
    HIP_TRY(fetch(c, argmin_out, e.argmin, N));
    HIP_TRY(fetch(c, min_out, a.fmin, N));
    HIP_TRY(fetch(c, center_objective_out, a.fcen, N));
    HIP_TRY(fetch(c, n_inside_out, a.cnt, N));
    if (intervals) {
        status.resize((size_t)N);
        HIP_TRY(fetch(c, status.data(), e.status, N));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (intervals) {                                      // failed centres are what cude_n_failed counts
        int64_t failed = 0;
        for (int64_t i = 0; i < N; i++) failed += (status[(size_t)i] & CUDE_CI_CENTER_FAILED) != 0;
        c->last_failed = failed;
        if (status_out) std::memcpy(status_out, status.data(), (size_t)N * sizeof(int32_t));
    }
    return CUDE_OK;
}

int32_t cude_fit_conditional(cude_ctx* c, double lower, double upper, int32_t n_grid, int32_t n_iters,
                             double penalty_weight, double penalty_center, double* cond_out, double* objective_out,
                             double* sse_out) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if (!c->have_pop) return fail(CUDE_ERR_STATE, "population not set");
    if (!c->have_nn) return fail(CUDE_ERR_STATE, "shared parameters not set");
    if (!(lower < upper) || !std::isfinite(lower) || !std::isfinite(upper)) return fail(CUDE_ERR_ARG, "need finite lower < upper");
    if (n_grid < 3 || n_iters < 1 || !(penalty_weight >= 0) || !std::isfinite(penalty_center))
        return fail(CUDE_ERR_ARG, "need n_grid >= 3, n_iters >= 1, penalty_weight >= 0");
    if (!cond_out) return fail(CUDE_ERR_ARG, "null output");
    const int64_t N = c->N;
    DevBuf<double> buf;                                   // a, b, c, d, fc, best, sse_c, sse_d
    HIP_TRY(buf.resize((size_t)8 * N));
    cude::FitArgs f{};
    f.N = N;
    f.a = buf.p; f.b = buf.p + N; f.c = buf.p + 2 * N; f.d = buf.p + 3 * N;
    f.fc = buf.p + 4 * N; f.best = buf.p + 5 * N;
    double* sse_c = buf.p + 6 * N;
    double* sse_d = buf.p + 7 * N;
    f.sse_c = sse_c; f.sse_d = sse_d;
    f.w = penalty_weight; f.mu = penalty_center;
    f.lower = lower; f.step = (upper - lower) / (n_grid - 1); f.gr = (std::sqrt(5.0) - 1.0) / 2.0;
    f.n_grid = n_grid;
    // Several probes per forward launch (option "fit_spec"): every launch below is one wave's whole solve per 64 subjects,
    // and a small population leaves the chip empty -- the grid values ride as parameter sets of one launch, and because a
    // golden-section step has two outcomes, the probes of the next d steps are a heap of 2^d - 1 brackets evaluated together
    // (cude_common.hip fit_tree_*).  The same expressions on the same values: the same brackets and result as the
    // one-probe-per-launch form, 138 forward launches -> 1 + 48 / d + 1.
    const bool fsplit = is_cpep(c) && !adaptive(c) && c->chunks > 1;
    const int fdepth = fit_spec_depth(c, fsplit);
    DevBuf<double> d_cand, d_sse, d_part, d_vals;          // (several probes per launch; alive until the final copies are in)
    if (fdepth >= 1) {
        const int P = c->P;
        const int64_t nb = c->nblocks;
        // sets per launch: the tree's, and for the grid scan as many as ~256 MB of per-set scratch allow
        const int tree_sets = 2 * ((1 << fdepth) - 1);
        const double per_set =
            8.0 * ((double)N * (2 + (fsplit ? (double)forward_chunks(c) * (3 + c->T) : 0.0)) + (double)nb * (P + 2));
        const int grid_sets = (int)sets_per_launch(n_grid, kNoGridCap, 256e6, per_set);
        const int max_sets = std::max(tree_sets, grid_sets);
        HIP_TRY(d_cand.resize((size_t)max_sets * N));
        HIP_TRY(d_sse.resize((size_t)max_sets * N));
        HIP_TRY(d_vals.resize((size_t)n_grid));
        if ((rc = reserve_sets_forward(c, max_sets, fsplit, d_part))) return rc;
        SetsForward fwd;                                      // SSE of every subject at cand[set][subject], one network
        fwd.cond = d_cand.p; fwd.nn = c->nn.p; fwd.sse = d_sse.p; fwd.partials = d_part.p; fwd.split = fsplit;
        std::vector<double> vals((size_t)n_grid);
        for (int k = 0; k < n_grid; k++) vals[k] = (k == n_grid - 1) ? upper : std::fma((double)k, f.step, lower);
        HIP_TRY(push(c, d_vals.p, vals.data(), n_grid));
        for (int k0 = 0; k0 < n_grid; k0 += grid_sets) {      // coarse scan of the box
            fwd.n_sets = std::min(grid_sets, n_grid - k0);
            HIP_TRY(cude::launch_fill_rows(N, fwd.n_sets, d_vals.p + k0, d_cand.p, c->stream));
            if ((rc = forward_sets(c, fwd))) return rc;
            HIP_TRY(cude::launch_fit_grid_all(f, k0, fwd.n_sets, d_vals.p, d_sse.p, c->stream));
            if (k0 == 0 && (rc = maybe_regroup(c))) return rc; // (adaptive mode: the first launch has told the step counts)
        }
        HIP_TRY(hipStreamSynchronize(c->stream));             // vals (host vector) was read by the copy above
        HIP_TRY(cude::launch_fit(1, f, 0, 0.0, c->stream));
        for (int it = 0; it < n_iters;) {                     // golden section inside the bracket, d steps per launch
            const int d = std::min(fdepth, n_iters - it);
            HIP_TRY(cude::launch_fit_tree(f, d, 0, 0, d_cand.p, d_sse.p, c->stream));
            fwd.n_sets = 2 * ((1 << d) - 1);
            if ((rc = forward_sets(c, fwd))) return rc;
            it += d;
            HIP_TRY(cude::launch_fit_tree(f, d, 1, it == n_iters ? 1 : 0, d_cand.p, d_sse.p, c->stream));
        }
    } else {
        // one probe per launch; everything is queued on the stream, the only synchronisation is the copy-back at the end
        for (int k = 0; k < n_grid; k++) {                    // coarse scan of the box
            const double x = (k == n_grid - 1) ? upper : std::fma((double)k, f.step, lower);
            HIP_TRY(cude::launch_fill(N, x, f.c, c->stream));
            if (k == 1 && (rc = maybe_regroup(c))) return rc;     // (adaptive mode: the first probe has told the step counts)
            if ((rc = run_ensemble(c, false, nullptr, true, f.c, sse_c))) return rc;
            HIP_TRY(cude::launch_fit(0, f, k, x, c->stream));
        }
        HIP_TRY(cude::launch_fit(1, f, 0, 0.0, c->stream));
        for (int it = 0; it < n_iters; it++) {                // golden section inside the bracket
            if ((rc = run_ensemble(c, false, nullptr, true, f.c, sse_c))) return rc;
            if ((rc = run_ensemble(c, false, nullptr, true, f.d, sse_d))) return rc;
            HIP_TRY(cude::launch_fit(2, f, it == n_iters - 1 ? 1 : 0, 0.0, c->stream));
        }
    }
    if ((rc = run_ensemble(c, false, nullptr, true, f.c, sse_c))) return rc;       // at the returned midpoint
    HIP_TRY(cude::launch_fit(3, f, 0, 0.0, c->stream));
    HIP_TRY(fetch(c, cond_out, f.c, N));
    HIP_TRY(fetch(c, objective_out, f.fc, N));
    HIP_TRY(fetch(c, sse_out, sse_c, N));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CUDE_OK;
}

int32_t cude_refine_conditional(cude_ctx* c, const double* x0, double lower, double upper, int32_t max_evals, double xtol,
                                double max_step, double penalty_weight, double penalty_center, double* cond_out,
                                double* objective_out, double* sse_out, double* info_out, int32_t* evals_out,
                                int32_t* status_out) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if (!c->have_pop) return fail(CUDE_ERR_STATE, "population not set");
    if (!c->have_nn) return fail(CUDE_ERR_STATE, "shared parameters not set");
    if (!x0 && !c->have_cond) return fail(CUDE_ERR_STATE, "no start: conditional parameters not set and x0 is null");
    if (!(lower < upper) || !std::isfinite(lower) || !std::isfinite(upper)) return fail(CUDE_ERR_ARG, "need finite lower < upper");
    if (max_evals < 1 || !(xtol > 0) || !(max_step > 0) || !(penalty_weight >= 0) || !std::isfinite(penalty_weight) ||
        !std::isfinite(penalty_center))
        return fail(CUDE_ERR_ARG, "need max_evals >= 1, xtol > 0, max_step > 0, finite penalty_weight >= 0");
    if (!cond_out) return fail(CUDE_ERR_ARG, "null output");
    if (c->net.generic())
        return fail(CUDE_ERR_UNSUPPORTED, "cude_refine_conditional: the network of this context runs on the fallback kernel "
                                          "(cude_set_network), which has no tangent-linear solve");
    if (c->capturing) return fail(CUDE_ERR_STATE, "cude_refine_conditional under stream capture");
    const bool cpep = is_cpep(c);
    const int64_t N = c->N;
    cude::RefineCfg k{};
    k.lower = lower; k.upper = upper; k.xtol = xtol; k.max_step = max_step;
    k.pw = penalty_weight; k.pc = penalty_center; k.max_evals = max_evals;
    cude::RefineArrays r{};
    double *sse_t = nullptr, *score_t = nullptr, *info_t = nullptr;
    if ((rc = refine_state(c, r, &sse_t, &score_t, &info_t))) return rc;
    if (x0) {
        HIP_TRY(push(c, c->refine_buf.p, x0, N));
        r.x0 = c->refine_buf.p;
    } else {
        r.x0 = c->cond.p;
    }
    hipError_t le = hipSuccess;
    if (!adaptive(c) && c->opt.refine_fused) {
        // the whole iteration of every subject in ONE launch
        if (cpep) {
            cude::CpepArgs a = cpep_args(c);
            a.nn = c->nn.p;
            le = cude::launch_cpep_refine(c->net, c->cfg.n_state, a, k, r, c->stream);
        } else {
            cude::SuppArgs a = supp_args(c);
            a.nn = c->nn.p;
            le = cude::launch_supp_refine(c->net, a, k, r, c->stream);
        }
    } else {
        le = refine_stepped(c, k, r, sse_t, score_t, info_t, nullptr);
    }
    if (le == hipErrorInvalidValue)
        return fail(CUDE_ERR_UNSUPPORTED, "cude_refine_conditional: no tangent kernel compiled for this network shape / model");
    HIP_TRY(le);
    // The SSE that is REPORTED is cude_forward's own at the returned point, as cude_fit_conditional's is (one forward launch
    // behind the iteration): the tangent sweep's SSE agrees with it to a few 1e-17 absolute, which on a near-perfect fit
    // (SSE ~ 1e-5) is 2e-12 relative -- callers compare these numbers across entry points.
    if ((rc = run_ensemble(c, false, nullptr, true, r.x, r.sse))) return rc;
    HIP_TRY(cude::launch_refine_step(2, k, r, c->stream));
    if (adaptive(c)) c->have_tape = false;
    std::vector<int32_t> status((size_t)N);
    HIP_TRY(fetch(c, cond_out, r.x, N));
    HIP_TRY(fetch(c, objective_out, r.F, N));
    HIP_TRY(fetch(c, sse_out, r.sse, N));
    HIP_TRY(fetch(c, info_out, r.info, N));
    HIP_TRY(fetch(c, evals_out, r.evals, N));
    HIP_TRY(fetch(c, status.data(), r.status, N));
    HIP_TRY(hipStreamSynchronize(c->stream));
    int64_t n_failed = 0;
    for (int64_t i = 0; i < N; i++) n_failed += status[(size_t)i] == CUDE_REFINE_FAILED;
    c->last_failed = n_failed;
    if (status_out) std::memcpy(status_out, status.data(), (size_t)N * sizeof(int32_t));
    return CUDE_OK;
}

}  // extern "C"
