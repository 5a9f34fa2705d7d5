// libcude_hip.so -- the entry points that simulate replicates of the data: the parametric bootstrap of the per-subject fits
// (cude_bootstrap_conditional), prediction discrepancies and npde (cude_npde), the visual predictive check by subject group
// (cude_vpc), and the read-backs of their device draws (cude_bootstrap_noise, cude_npde_draws).  cude_npde and cude_vpc are
// one pipeline -- sets, solve at the data's times, noise, observations: simulate_observe_pass -- walked in two directions:
// all simulations of a block of subjects, all subjects of a block of simulations.
#include "cude_ctx.h"

using namespace cude::api;

int32_t SimObserve::prepare(cude_ctx* c, const double* sigma, int64_t sets_max, int64_t sub_max, int64_t blocks) {
    const bool cpep = is_cpep(c);
    const int64_t N = c->N;
    const int T = c->T, R = T - 1, NS = cpep ? c->cfg.n_state : 3;
    HIP_TRY(d_cond.resize((size_t)sets_max * N));
    HIP_TRY(d_sigma.resize((size_t)N));
    HIP_TRY(d_slab.resize((size_t)sets_max * sub_max * T * NS));
    HIP_TRY(d_y.resize((size_t)sets_max * R * sub_max));
    HIP_TRY(d_used.resize((size_t)sets_max * sub_max));
    if (cpep || adaptive(c)) HIP_TRY(d_part.resize((size_t)sets_max * blocks * (c->P + 2)));
    HIP_TRY(push(c, d_sigma.p, sigma, N));
    return tables.upload(c, T, c->tp.data());
}

int32_t cude::api::simulate_observe_pass(cude_ctx* c, const SimObserve& v, int64_t s0, int64_t sn, int64_t k0, int64_t kn,
                                         bool place) {
    int32_t rc = CUDE_OK;
    const bool cpep = is_cpep(c);
    const int64_t N = c->N;
    const int T = c->T, R = T - 1, NS = cpep ? c->cfg.n_state : 3;
    if (place && v.cond_sets) HIP_TRY(push(c, v.d_cond.p, v.cond_sets + (size_t)k0 * N, (size_t)kn * N));
    else if (place) {
        cude::NpdePlaceArgs pl{};
        pl.N = N; pl.K = (int32_t)kn; pl.normals_only = 0; pl.prior_mean = v.prior_mean; pl.prior_sd = v.prior_sd;
        pl.seed = c->rng_seed; pl.subject_offset = c->rng_offset; pl.first_rep = v.first_rep + k0; pl.out = v.d_cond.p;
        HIP_TRY(cude::launch_npde_place(pl, c->stream));
    }
    DenseLaunch d;                                        // kn sets at the data's own times; the caller's order of subjects
    d.cond = v.d_cond.p; d.n_sets = (int32_t)kn; d.partials = v.d_part.p; d.keep_perm = false;
    d.traj_ss = 1; d.traj_st = 3; d.traj_sn = 3 * T;
    d.k0 = 0; d.kn = T;
    d.set_stride = (int64_t)NS * T * sn;
    d.blk_first = s0 / cude::kBlock; d.blk_count = (sn + cude::kBlock - 1) / cude::kBlock;
    // subject i of the population writes column block (i - s0) of the slab
    d.traj = v.d_slab.p - (int64_t)NS * T * s0;
    // outputs a failed adaptive solve does not reach stay NaN
    if (adaptive(c)) HIP_TRY(hipMemsetAsync(v.d_slab.p, 0xff, (size_t)kn * d.set_stride * sizeof(double), c->stream));
    if ((rc = launch_dense(c, v.tables, d))) return rc;
    // the caller's noise of these simulations and subjects goes into the table of simulated observations and is turned into
    // them in place
    if (v.noise)
        HIP_TRY(hipMemcpy2DAsync(v.d_y.p, (size_t)sn * sizeof(double), v.noise + (size_t)k0 * R * N + s0, (size_t)N * sizeof(double),
                                 (size_t)sn * sizeof(double), (size_t)kn * R, hipMemcpyHostToDevice, c->stream));
    cude::NpdeObserveArgs oa{};
    oa.K = (int32_t)kn; oa.T = T; oa.NS = NS; oa.state = v.state; oa.from_noise = v.noise ? 1 : 0;
    oa.scale = cpep ? 1.0 : c->scale[v.state];
    oa.slab = v.d_slab.p; oa.sigma = v.d_sigma.p; oa.y = v.d_y.p; oa.used = v.d_used.p;
    oa.seed = c->rng_seed; oa.subject_offset = c->rng_offset; oa.first_rep = v.first_rep + k0;
    oa.subj0 = s0; oa.n_subj = sn;
    HIP_TRY(cude::launch_npde_observe(oa, c->stream));
    return CUDE_OK;
}

namespace {
// Replicates per launch of the bootstrap's observations and of either read-back of draws: ~256 MB of [rows][N] each
int64_t draws_chunk(const cude_ctx* c, int64_t n, int rows, int option_cap) {
    return sets_per_launch(n, 65535, 256e6, 8.0 * rows * (double)c->N, option_cap);
}

// Device draws read back: draw(k0, kn, buf) queues the launch that writes replicates [k0, k0 + kn) as [kn][rows][N]
template <class Draw>
int32_t fetch_draws(cude_ctx* c, int64_t n, int rows, int option_cap, double* out, Draw draw) {
    const size_t per_rep = (size_t)rows * c->N;
    const int64_t chunk = draws_chunk(c, n, rows, option_cap);
    DevBuf<double> d_eps;
    HIP_TRY(d_eps.resize((size_t)chunk * per_rep));
    for (int64_t k0 = 0; k0 < n; k0 += chunk) {
        const int64_t kn = std::min<int64_t>(chunk, n - k0);
        HIP_TRY(draw(k0, kn, d_eps.p));
        HIP_TRY(fetch(c, out + (size_t)k0 * per_rep, d_eps.p, (size_t)kn * per_rep));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return CUDE_OK;
}

// What cude_npde and cude_vpc check alike, in two stretches (each has checks of its own between them); `name`: the entry point
int32_t check_simulation(const cude_ctx* c, const char* name, int32_t n_sims, int64_t first_rep, int32_t state,
                         const double* cond_sets, double prior_mean, double prior_sd) {
    if (!c->have_pop) return fail(CUDE_ERR_STATE, "population not set");
    if (!c->have_nn) return fail(CUDE_ERR_STATE, "shared parameters not set");
    if (c->net.generic())
        return fail(CUDE_ERR_UNSUPPORTED, std::string(name) + ": the network of this context runs on the fallback kernel "
                                                              "(cude_set_network), whose dense output takes one parameter set");
    if (c->capturing) return fail(CUDE_ERR_STATE, std::string(name) + " under stream capture");
    if (n_sims < 2 || n_sims > cude::kPredMaxSets) return fail(CUDE_ERR_ARG, "need 2 <= n_sims <= 4096");
    if (first_rep < 0 || first_rep > cude::kRngMaxReplicate - n_sims) return fail(CUDE_ERR_ARG, "need 0 <= first_rep, first_rep + n_sims <= 2^47");
    if (state < 0 || state >= (is_cpep(c) ? 1 : 3)) return fail(CUDE_ERR_ARG, "state out of range (c-peptide models: 0, the observed state)");
    if (!cond_sets && (!(prior_sd > 0) || !std::isfinite(prior_sd) || !std::isfinite(prior_mean)))
        return fail(CUDE_ERR_ARG, "need finite prior_mean and prior_sd > 0 when cond_sets is null");
    return CUDE_OK;
}
// ... sigma, subject by subject together with cude_vpc's group ids (group: null for cude_npde), and the data's rows
int32_t check_sigma_and_rows(const cude_ctx* c, const double* sigma, const int32_t* group, int32_t n_groups) {
    if (!sigma) return fail(CUDE_ERR_ARG, "null sigma");
    for (int64_t i = 0; i < c->N; i++) {
        if (sigma[i] < 0) return fail(CUDE_ERR_ARG, "sigma must not be negative");
        if (group && group[i] >= n_groups) return fail(CUDE_ERR_ARG, "group id >= n_groups");
    }
    if (c->T - 1 < 1) return fail(CUDE_ERR_ARG, "the population has no data time after t_0");
    return CUDE_OK;
}
}  // namespace

extern "C" {

int32_t cude_bootstrap_conditional(cude_ctx* c, const double* center, const double* sigma, int64_t first_rep, int32_t n_reps,
                                   const double* noise, double lower, double upper, int32_t max_evals, double xtol,
                                   double max_step, double penalty_weight, double penalty_center, int32_t n_ranks,
                                   const int32_t* ranks, double* order_out, double* mean_out, double* sd_out,
                                   int32_t* n_used_out, double* reps_out, int32_t* status_out) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if (!c->have_pop) return fail(CUDE_ERR_STATE, "population not set");
    if (!c->have_nn) return fail(CUDE_ERR_STATE, "shared parameters not set");
    if (!center && !c->have_cond) return fail(CUDE_ERR_STATE, "no centre: conditional parameters not set and center is null");
    if (!(lower < upper) || !std::isfinite(lower) || !std::isfinite(upper)) return fail(CUDE_ERR_ARG, "need finite lower < upper");
    if (max_evals < 1 || !(xtol > 0) || !(max_step > 0) || !(penalty_weight >= 0) || !std::isfinite(penalty_weight) ||
        !std::isfinite(penalty_center))
        return fail(CUDE_ERR_ARG, "need max_evals >= 1, xtol > 0, max_step > 0, finite penalty_weight >= 0");
    if (n_reps < 1 || n_reps > cude::kPredMaxSets) return fail(CUDE_ERR_ARG, "need 1 <= n_reps <= 4096");
    if (first_rep < 0 || first_rep > cude::kRngMaxReplicate - n_reps) return fail(CUDE_ERR_ARG, "need 0 <= first_rep, first_rep + n_reps <= 2^47");
    if (n_ranks < 0 || n_ranks > cude::kPredMaxRanks) return fail(CUDE_ERR_ARG, "need 0 <= n_ranks <= 16");
    if ((n_ranks > 0 && (!ranks || !order_out)) || (n_ranks == 0 && order_out))
        return fail(CUDE_ERR_ARG, "need order_out with n_ranks > 0 ranks, and only then");
    if (!order_out && !mean_out && !sd_out && !n_used_out && !reps_out && !status_out) return fail(CUDE_ERR_ARG, "no output requested");
    if (!ranks_increasing(n_ranks, ranks, n_reps)) return fail(CUDE_ERR_ARG, "ranks must be strictly increasing inside [0, n_reps)");
    if (!sigma) return fail(CUDE_ERR_ARG, "null sigma");
    const int64_t N = c->N, nb = c->nblocks;
    for (int64_t i = 0; i < N; i++)
        if (!(sigma[i] >= 0) || !std::isfinite(sigma[i])) return fail(CUDE_ERR_ARG, "sigma must be finite and >= 0");
    if (c->net.generic())
        return fail(CUDE_ERR_UNSUPPORTED, "cude_bootstrap_conditional: the network of this context runs on the fallback kernel "
                                          "(cude_set_network), which has no tangent-linear solve");
    if (c->capturing) return fail(CUDE_ERR_STATE, "cude_bootstrap_conditional under stream capture");
    const bool cpep = is_cpep(c);
    const int T = c->T, n_states = cpep ? 1 : 3, rows = n_states * T;
    const bool fused = !adaptive(c) && c->opt.refine_fused;
    // Replicates per launch: ~256 MB of replicate observations ([rows][N] each).  Subjects per pass: whole workgroups, as many
    // as ~1 GB of replicate results (a double and an int32 per replicate and subject) allow.
    const int64_t chunk = draws_chunk(c, n_reps, rows, c->opt.bootstrap_chunk);
    const SubjectPasses passes = subject_passes(N, nb, cude::kBlock, 1e9, 12.0 * n_reps * cude::kBlock, c->opt.bootstrap_subjects);
    const int64_t sub_max = passes.sub_max;
    DevBuf<double> d_in, d_slab, d_reps, d_sum;
    DevBuf<int32_t> d_status, d_int;
    HIP_TRY(d_in.resize((size_t)3 * N));                  // centre, sigma, the SSE of the centre's solve (not reported)
    HIP_TRY(d_slab.resize((size_t)chunk * rows * N));
    HIP_TRY(d_reps.resize((size_t)n_reps * sub_max));
    HIP_TRY(d_status.resize((size_t)n_reps * sub_max));
    HIP_TRY(d_sum.resize((size_t)(n_ranks + 2) * sub_max));        // order [n_ranks][sub_max], mean, sd
    HIP_TRY(d_int.resize((size_t)sub_max + (size_t)std::max(n_ranks, 1)));      // n_used, ranks
    double* const d_center = d_in.p;
    double* const d_sigma = d_in.p + N;
    double* const d_order = d_sum.p;
    double* const d_mean = d_sum.p + (size_t)n_ranks * sub_max;
    double* const d_sd = d_mean + sub_max;
    int32_t* const d_used = d_int.p;
    int32_t* const d_ranks = d_int.p + sub_max;
    if (center) HIP_TRY(push(c, d_center, center, N));
    else HIP_TRY(hipMemcpyAsync(d_center, c->cond.p, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(push(c, d_sigma, sigma, N));
    if (n_ranks > 0) HIP_TRY(push(c, d_ranks, ranks, n_ranks));
    // rule 1: cude_forward's trajectory at the centre
    HIP_TRY(c->traj.resize((size_t)c->cfg.n_state * T * N));
    if ((rc = run_ensemble(c, false, c->traj.p, true, d_center, d_in.p + 2 * N))) return rc;
    if (adaptive(c)) c->have_tape = false;
    cude::BootstrapGenArgs g{};
    g.N = N; g.T = T; g.n_states = n_states; g.traj_states = c->cfg.n_state;
    for (int s = 0; s < 3; s++) g.scale[s] = cpep ? 1.0 : c->scale[s];
    g.traj = c->traj.p; g.sigma = d_sigma; g.pop = cpep ? c->obs.p : c->data.p;
    g.slab = d_slab.p; g.from_noise = noise ? 1 : 0;
    g.seed = c->rng_seed; g.subject_offset = c->rng_offset;
    cude::RefineCfg k{};
    k.lower = lower; k.upper = upper; k.xtol = xtol; k.max_step = max_step;
    k.pw = penalty_weight; k.pc = penalty_center; k.max_evals = max_evals;
    cude::RefineArrays r{};
    double *sse_t = nullptr, *score_t = nullptr, *info_t = nullptr;
    if (fused) r.N = N;
    else if ((rc = refine_state(c, r, &sse_t, &score_t, &info_t))) return rc;
    r.x0 = d_center;
    std::vector<int32_t> used((size_t)N);
    const size_t pitch_host = (size_t)N * sizeof(double), pitch_dev = (size_t)sub_max * sizeof(double);
    for (int64_t b = 0; b < nb; b += passes.blocks) {
        const auto [b0, bn, s0, sn] = passes.at(b);
        g.subj0 = s0; g.n_subj = sn;
        for (int64_t k0 = 0; k0 < n_reps; k0 += chunk) {
            const int64_t kn = std::min<int64_t>(chunk, n_reps - k0);
            g.n_reps = (int32_t)kn; g.first_rep = first_rep + k0;
            // the caller's noise of these subjects goes into the slab itself and is turned into observations in place
            if (noise)
                HIP_TRY(hipMemcpy2DAsync(d_slab.p + s0, pitch_host, noise + (size_t)k0 * rows * N + s0, pitch_host,
                                         (size_t)sn * sizeof(double), (size_t)kn * rows, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(cude::launch_bootstrap_generate(g, c->stream));
            hipError_t le = hipSuccess;
            if (fused) {
                // every fit of the chunk in ONE launch: workgroup (x, y) = subjects 64 (b0 + x) ... of replicate k0 + y
                cude::RefineReps p{};
                p.slab = d_slab.p; p.slab_stride = (int64_t)rows * N; p.rep_stride = sub_max;
                p.blk_first = b0; p.blk_count = bn; p.n_reps = (int32_t)kn;
                r.x = d_reps.p + k0 * sub_max - s0;
                r.status = d_status.p + k0 * sub_max - s0;
                if (cpep) {
                    cude::CpepArgs a = cpep_args(c);
                    a.nn = c->nn.p;
                    le = cude::launch_cpep_refine(c->net, c->cfg.n_state, a, k, r, c->stream, &p);
                } else {
                    cude::SuppArgs a = supp_args(c);
                    a.nn = c->nn.p;
                    le = cude::launch_supp_refine(c->net, a, k, r, c->stream, &p);
                }
            } else {
                // the stepped form, one replicate at a time over the whole population: max_evals tangent launches each
                for (int64_t j = 0; j < kn && le == hipSuccess; j++) {
                    le = refine_stepped(c, k, r, sse_t, score_t, info_t, d_slab.p + j * rows * N);
                    if (le != hipSuccess) break;
                    HIP_TRY(hipMemcpyAsync(d_reps.p + (k0 + j) * sub_max, r.x + s0, (size_t)sn * sizeof(double),
                                           hipMemcpyDeviceToDevice, c->stream));
                    HIP_TRY(hipMemcpyAsync(d_status.p + (k0 + j) * sub_max, r.status + s0, (size_t)sn * sizeof(int32_t),
                                           hipMemcpyDeviceToDevice, c->stream));
                }
            }
            if (le == hipErrorInvalidValue)
                return fail(CUDE_ERR_UNSUPPORTED, "cude_bootstrap_conditional: no tangent kernel compiled for this network shape / model");
            HIP_TRY(le);
        }
        // rule 5, over all replicates of these subjects
        cude::BootstrapReduceArgs ra{};
        ra.reps = d_reps.p; ra.status = d_status.p; ra.stride = sub_max; ra.n_subj = sn;
        ra.K = n_reps; ra.n_ranks = n_ranks;
        ra.order = n_ranks > 0 ? d_order : nullptr; ra.out_stride = sub_max;
        ra.mean = d_mean; ra.sd = d_sd; ra.n_used = d_used;
        HIP_TRY(cude::launch_bootstrap_reduce(ra, d_ranks, c->stream));
        if (order_out)
            HIP_TRY(hipMemcpy2DAsync(order_out + s0, pitch_host, d_order, pitch_dev, (size_t)sn * sizeof(double), (size_t)n_ranks,
                                     hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(fetch(c, mean_out ? mean_out + s0 : nullptr, d_mean, sn));
        HIP_TRY(fetch(c, sd_out ? sd_out + s0 : nullptr, d_sd, sn));
        HIP_TRY(fetch(c, used.data() + s0, d_used, sn));
        if (reps_out)
            HIP_TRY(hipMemcpy2DAsync(reps_out + s0, pitch_host, d_reps.p, pitch_dev, (size_t)sn * sizeof(double), (size_t)n_reps,
                                     hipMemcpyDeviceToHost, c->stream));
        if (status_out)
            HIP_TRY(hipMemcpy2DAsync(status_out + s0, (size_t)N * sizeof(int32_t), d_status.p, (size_t)sub_max * sizeof(int32_t),
                                     (size_t)sn * sizeof(int32_t), (size_t)n_reps, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));         // the result tables are the next pass's too
    }
    int64_t failed = 0;
    for (int64_t i = 0; i < N; i++) failed += used[(size_t)i] < n_reps;
    c->last_failed = failed;
    if (n_used_out) std::memcpy(n_used_out, used.data(), (size_t)N * sizeof(int32_t));
    return CUDE_OK;
}

int32_t cude_bootstrap_noise(cude_ctx* c, int64_t first_rep, int32_t n_reps, double* noise_out) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if (!c->have_pop) return fail(CUDE_ERR_STATE, "population not set");
    if (n_reps < 1 || n_reps > cude::kPredMaxSets) return fail(CUDE_ERR_ARG, "need 1 <= n_reps <= 4096");
    if (first_rep < 0 || first_rep > cude::kRngMaxReplicate - n_reps) return fail(CUDE_ERR_ARG, "need 0 <= first_rep, first_rep + n_reps <= 2^47");
    if (!noise_out) return fail(CUDE_ERR_ARG, "null output");
    if (c->capturing) return fail(CUDE_ERR_STATE, "cude_bootstrap_noise under stream capture");
    const int64_t N = c->N;
    const int T = c->T, n_states = is_cpep(c) ? 1 : 3, rows = n_states * T;
    cude::BootstrapGenArgs g{};
    g.N = N; g.subj0 = 0; g.n_subj = N; g.T = T; g.n_states = n_states;
    g.seed = c->rng_seed; g.subject_offset = c->rng_offset;
    return fetch_draws(c, n_reps, rows, c->opt.bootstrap_chunk, noise_out, [&](int64_t k0, int64_t kn, double* d_eps) {
        g.n_reps = (int32_t)kn; g.first_rep = first_rep + k0;
        return cude::launch_bootstrap_noise(g, d_eps, c->stream);
    });
}

int32_t cude_npde(cude_ctx* c, int32_t n_sims, const double* cond_sets, double prior_mean, double prior_sd, const double* sigma,
                  int64_t first_rep, const double* noise, int32_t state, double* pred_mean_out, double* pred_var_out,
                  int32_t* below_out, int32_t* below_decorr_out, double* pd_out, double* npde_out, int32_t* n_used_out,
                  int32_t* status_out, double* sims_out) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if ((rc = check_simulation(c, "cude_npde", n_sims, first_rep, state, cond_sets, prior_mean, prior_sd))) return rc;
    if (!pred_mean_out && !pred_var_out && !below_out && !below_decorr_out && !pd_out && !npde_out && !n_used_out && !status_out &&
        !sims_out)
        return fail(CUDE_ERR_ARG, "no output requested");
    if ((rc = check_sigma_and_rows(c, sigma, nullptr, 0))) return rc;
    const bool cpep = is_cpep(c);
    const int NS = cpep ? c->cfg.n_state : 3;
    const int64_t N = c->N, K = n_sims, nb = c->nblocks;
    const int T = c->T, R = T - 1;
    // Subjects per pass: whole workgroups, as many as ~1 GB of trajectories ([K][subjects][T][NS]), simulated observations
    // ([K][R][subjects]) and their flags allow -- all K simulations of a subject are resident when it is reduced
    const double per_block = ((8.0 * NS * T + 8.0 * R + 1.0) * (double)K) * cude::kBlock;
    const SubjectPasses passes = subject_passes(N, nb, cude::kBlock, 1e9, per_block, c->opt.npde_subjects);
    SimObserve sim;
    sim.cond_sets = cond_sets; sim.prior_mean = prior_mean; sim.prior_sd = prior_sd; sim.noise = noise;
    sim.first_rep = first_rep; sim.state = state;
    DevBuf<double> d_out;
    DevBuf<int32_t> d_int;
    HIP_TRY(d_out.resize((size_t)4 * R * N));            // pred_mean, pred_var, pd, npde: [R][N] each
    HIP_TRY(d_int.resize((size_t)(2 * R + 2) * N + 1));   // below, below_decorr [R][N]; n_used, status [N]; failed subjects
    cude::NpdeReduceArgs ra{};
    ra.N = N; ra.K = (int32_t)K; ra.R = R;
    ra.obs = cpep ? c->obs.p : c->data.p + (size_t)state * T * N;
    ra.pred_mean = d_out.p; ra.pred_var = d_out.p + (size_t)R * N; ra.pd = d_out.p + (size_t)2 * R * N;
    ra.npde = d_out.p + (size_t)3 * R * N;
    ra.below = d_int.p; ra.below_decorr = d_int.p + (size_t)R * N;
    ra.n_used = d_int.p + (size_t)2 * R * N; ra.status = ra.n_used + N; ra.n_failed = ra.status + N;
    if (!below_decorr_out && !npde_out) { ra.below_decorr = nullptr; ra.npde = nullptr; }     // (the substitution is skipped)
    HIP_TRY(hipMemsetAsync(ra.n_failed, 0, sizeof(int32_t), c->stream));
    if ((rc = sim.prepare(c, sigma, K, passes.sub_max, passes.blocks))) return rc;
    ra.y = sim.d_y.p; ra.used = sim.d_used.p; ra.sigma = sim.d_sigma.p;
    for (int64_t b = 0; b < nb; b += passes.blocks) {
        const auto [b0, bn, s0, sn] = passes.at(b);
        // all K simulations of these subjects; the sets (every subject's) are placed once, by the first pass
        if ((rc = simulate_observe_pass(c, sim, s0, sn, 0, K, b == 0))) return rc;
        ra.subj0 = s0; ra.n_subj = sn;
        HIP_TRY(cude::launch_npde_reduce(ra, c->stream));
        if (sims_out)
            HIP_TRY(hipMemcpy2DAsync(sims_out + s0, (size_t)N * sizeof(double), sim.d_y.p, (size_t)sn * sizeof(double),
                                     (size_t)sn * sizeof(double), (size_t)K * R, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));         // the slab and the tables are the next pass's too
    }
    int32_t failed = 0;
    HIP_TRY(fetch(c, pred_mean_out, d_out.p, (size_t)R * N));
    HIP_TRY(fetch(c, pred_var_out, d_out.p + (size_t)R * N, (size_t)R * N));
    HIP_TRY(fetch(c, pd_out, d_out.p + (size_t)2 * R * N, (size_t)R * N));
    HIP_TRY(fetch(c, npde_out, d_out.p + (size_t)3 * R * N, (size_t)R * N));
    HIP_TRY(fetch(c, below_out, d_int.p, (size_t)R * N));
    HIP_TRY(fetch(c, below_decorr_out, d_int.p + (size_t)R * N, (size_t)R * N));
    HIP_TRY(fetch(c, n_used_out, d_int.p + (size_t)2 * R * N, N));
    HIP_TRY(fetch(c, status_out, d_int.p + (size_t)(2 * R + 1) * N, N));
    HIP_TRY(fetch(c, &failed, d_int.p + (size_t)(2 * R + 2) * N, 1));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->last_failed = failed;
    return CUDE_OK;
}

int32_t cude_npde_draws(cude_ctx* c, int64_t first_rep, int32_t n_sims, double* eta_normals_out, double* noise_out) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if (!c->have_pop) return fail(CUDE_ERR_STATE, "population not set");
    if (n_sims < 1 || n_sims > cude::kPredMaxSets) return fail(CUDE_ERR_ARG, "need 1 <= n_sims <= 4096");
    if (first_rep < 0 || first_rep > cude::kRngMaxReplicate - n_sims) return fail(CUDE_ERR_ARG, "need 0 <= first_rep, first_rep + n_sims <= 2^47");
    if (!eta_normals_out && !noise_out) return fail(CUDE_ERR_ARG, "null output");
    if (c->capturing) return fail(CUDE_ERR_STATE, "cude_npde_draws under stream capture");
    const int64_t N = c->N;
    const int T = c->T, R = T - 1;
    if (noise_out && R < 1) return fail(CUDE_ERR_ARG, "the population has no data time after t_0");
    if (eta_normals_out) {
        DevBuf<double> d_z;
        HIP_TRY(d_z.resize((size_t)n_sims * N));
        cude::NpdePlaceArgs pl{};
        pl.N = N; pl.K = n_sims; pl.normals_only = 1;
        pl.seed = c->rng_seed; pl.subject_offset = c->rng_offset; pl.first_rep = first_rep; pl.out = d_z.p;
        HIP_TRY(cude::launch_npde_place(pl, c->stream));
        HIP_TRY(fetch(c, eta_normals_out, d_z.p, (size_t)n_sims * N));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (noise_out) {
        cude::NpdeObserveArgs oa{};
        oa.subj0 = 0; oa.n_subj = N; oa.T = T; oa.noise_only = 1;
        oa.seed = c->rng_seed; oa.subject_offset = c->rng_offset;
        return fetch_draws(c, n_sims, R, 0, noise_out, [&](int64_t k0, int64_t kn, double* d_eps) {
            oa.K = (int32_t)kn; oa.first_rep = first_rep + k0; oa.y = d_eps;
            return cude::launch_npde_observe(oa, c->stream);
        });
    }
    return CUDE_OK;
}

int32_t cude_vpc(cude_ctx* c, int32_t n_sims, const double* cond_sets, double prior_mean, double prior_sd, const double* sigma,
                 int64_t first_rep, const double* noise, int32_t state, int32_t n_groups, const int32_t* group, int32_t n_levels,
                 const double* levels, int32_t n_ci, const double* ci_levels, double* obs_q_out, double* sim_ci_out,
                 double* sim_q_out, int32_t* n_members_out, int32_t* n_sims_used_out, int32_t* status_out) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if ((rc = check_simulation(c, "cude_vpc", n_sims, first_rep, state, cond_sets, prior_mean, prior_sd))) return rc;
    if (!obs_q_out && !sim_ci_out && !sim_q_out) return fail(CUDE_ERR_ARG, "none of obs_q_out, sim_ci_out, sim_q_out requested");
    if (n_groups < 1 || n_groups > cude::kVpcMaxGroups) return fail(CUDE_ERR_ARG, "need 1 <= n_groups <= 8");
    const auto increasing = [](int32_t n, const double* q) {
        if (n < 1 || n > cude::kVpcMaxLevels || !q) return false;
        for (int i = 0; i < n; i++)
            if (!(q[i] >= 0.0 && q[i] <= 1.0) || (i > 0 && !(q[i] > q[i - 1]))) return false;
        return true;
    };
    if (!increasing(n_levels, levels)) return fail(CUDE_ERR_ARG, "need 1 <= n_levels <= 8 levels, strictly increasing inside [0, 1]");
    if (!increasing(n_ci, ci_levels)) return fail(CUDE_ERR_ARG, "need 1 <= n_ci <= 8 ci_levels, strictly increasing inside [0, 1]");
    if ((rc = check_sigma_and_rows(c, sigma, group, n_groups))) return rc;
    const bool cpep = is_cpep(c);
    const int NS = cpep ? c->cfg.n_state : 3;
    const int64_t N = c->N, K = n_sims, nb = c->nblocks;
    const int T = c->T, R = T - 1, G = n_groups, L = n_levels, C = n_ci;
    // Simulations per pass: as many as ~1 GB of trajectories ([sims][N][T][NS]), simulated observations ([sims][R][N]) and
    // their flags allow -- all N subjects of a simulation are resident when it is reduced
    const double per_sim = (8.0 * NS * T + 8.0 * R + 1.0) * (double)nb * cude::kBlock;
    const int64_t chunk = sets_per_launch(K, 65535, 1e9, per_sim, c->opt.vpc_sims);
    const size_t GRL = (size_t)G * R * L;
    SimObserve sim;
    sim.cond_sets = cond_sets; sim.prior_mean = prior_mean; sim.prior_sd = prior_sd; sim.noise = noise;
    sim.first_rep = first_rep; sim.state = state;
    DevBuf<double> d_q, d_lev;
    DevBuf<int32_t> d_int;
    DevBuf<uint8_t> d_bad, d_simbad;
    if ((rc = sim.prepare(c, sigma, chunk, N, nb))) return rc;
    HIP_TRY(d_bad.resize((size_t)N));
    HIP_TRY(d_simbad.resize((size_t)K * G));
    HIP_TRY(d_q.resize((size_t)(K + 1 + C) * GRL));        // sim_q [K][G][R][L], obs_q [G][R][L], sim_ci [G][R][L][C]
    HIP_TRY(d_lev.resize((size_t)(L + C)));
    HIP_TRY(d_int.resize((size_t)3 * N + 2 * G));          // the strata, their member lists, status [N]; n_members, n_used [G]
    double* const d_simq = d_q.p;
    double* const d_obsq = d_q.p + (size_t)K * GRL;
    double* const d_ci = d_obsq + GRL;
    int32_t* const d_grp = d_int.p;
    int32_t* const d_members = d_int.p + N;
    int32_t* const d_status = d_int.p + 2 * N;
    int32_t* const d_nmem = d_int.p + 3 * N;
    int32_t* const d_nused = d_nmem + G;
    const double* const obs = cpep ? c->obs.p : c->data.p + (size_t)state * T * N;
    // ---- rule 2: the members of every stratum, in subject order (the host knows the ids; the device the observations)
    HIP_TRY(push(c, d_lev.p, levels, L));
    HIP_TRY(push(c, d_lev.p + L, ci_levels, C));
    HIP_TRY(cude::launch_vpc_bad_obs(N, R, obs, sim.d_sigma.p, d_bad.p, c->stream));
    std::vector<uint8_t> bad((size_t)N);
    HIP_TRY(fetch(c, bad.data(), d_bad.p, N));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<int32_t> grp((size_t)N), status((size_t)N), members, first((size_t)G + 1, 0), n_members((size_t)G, 0);
    for (int64_t i = 0; i < N; i++) {
        const int32_t g = group ? group[i] : 0;
        status[(size_t)i] = g < 0 ? CUDE_VPC_NO_GROUP : (bad[(size_t)i] ? CUDE_VPC_BAD_OBS : 0);
        grp[(size_t)i] = status[(size_t)i] ? -1 : g;
        if (grp[(size_t)i] >= 0) n_members[(size_t)g]++;
    }
    for (int g = 0; g < G; g++) first[(size_t)g + 1] = first[(size_t)g] + n_members[(size_t)g];
    members.resize((size_t)std::max<int32_t>(1, first[(size_t)G]));
    {
        std::vector<int32_t> at(first.begin(), first.end() - 1);
        for (int64_t i = 0; i < N; i++)
            if (grp[(size_t)i] >= 0) members[(size_t)at[(size_t)grp[(size_t)i]]++] = (int32_t)i;
    }
    HIP_TRY(push(c, d_grp, grp.data(), N));
    if (first[(size_t)G] > 0) HIP_TRY(push(c, d_members, members.data(), (size_t)first[(size_t)G]));
    HIP_TRY(push(c, d_status, status.data(), N));
    HIP_TRY(push(c, d_nmem, n_members.data(), G));
    HIP_TRY(hipMemsetAsync(d_simbad.p, 0, (size_t)K * G, c->stream));
    const bool force_select = c->opt.vpc_select != 0;
    cude::VpcColumnsArgs ca{};
    ca.N = N; ca.R = R; ca.G = G; ca.L = L; ca.levels = d_lev.p;
    // ---- rule 4: the observations as one more "simulation" (rows t_1 ... of the population's table [T][N])
    for (int g = 0; g < G && obs_q_out; g++) {
        ca.y = obs + N; ca.K = 1; ca.sim_bad = nullptr; ca.out = d_obsq;
        ca.g = g; ca.members = d_members + first[(size_t)g]; ca.n = n_members[(size_t)g];
        HIP_TRY(cude::launch_vpc_columns(ca, force_select, c->stream));
    }
    // ---- rules 1 and 5, pass by pass
    for (int64_t k0 = 0; k0 < K; k0 += chunk) {
        const int64_t kn = std::min<int64_t>(chunk, K - k0);
        // all N subjects of these simulations, whose sets are placed pass by pass
        if ((rc = simulate_observe_pass(c, sim, 0, N, k0, kn, true))) return rc;
        HIP_TRY(cude::launch_vpc_flag(N, (int)kn, G, d_grp, sim.d_used.p, d_simbad.p + (size_t)k0 * G, d_status, c->stream));
        for (int g = 0; g < G; g++) {
            ca.y = sim.d_y.p; ca.K = (int32_t)kn; ca.sim_bad = d_simbad.p + (size_t)k0 * G; ca.out = d_simq + (size_t)k0 * GRL;
            ca.g = g; ca.members = d_members + first[(size_t)g]; ca.n = n_members[(size_t)g];
            HIP_TRY(cude::launch_vpc_columns(ca, force_select, c->stream));
        }
        HIP_TRY(hipStreamSynchronize(c->stream));         // the slab, the sets and the tables are the next pass's too
    }
    // ---- rule 6
    HIP_TRY(cude::launch_vpc_count((int)K, G, d_simbad.p, d_nused, c->stream));
    if (sim_ci_out) {
        cude::VpcIntervalArgs ia{};
        ia.sim_q = d_simq; ia.sim_bad = d_simbad.p; ia.n_used = d_nused; ia.n_members = d_nmem;
        ia.K = (int32_t)K; ia.G = G; ia.R = R; ia.L = L; ia.C = C; ia.ci_levels = d_lev.p + L; ia.ci = d_ci;
        HIP_TRY(cude::launch_vpc_interval(ia, c->stream));
    }
    HIP_TRY(fetch(c, obs_q_out, d_obsq, GRL));
    HIP_TRY(fetch(c, sim_ci_out, d_ci, GRL * C));
    HIP_TRY(fetch(c, sim_q_out, d_simq, (size_t)K * GRL));
    HIP_TRY(fetch(c, n_sims_used_out, d_nused, G));
    HIP_TRY(fetch(c, status.data(), d_status, N));
    HIP_TRY(hipStreamSynchronize(c->stream));
    int64_t failed = 0;
    for (int64_t i = 0; i < N; i++) failed += (status[(size_t)i] & (CUDE_VPC_BAD_OBS | CUDE_VPC_FAILED_SIMS)) != 0;
    c->last_failed = failed;
    if (n_members_out) std::memcpy(n_members_out, n_members.data(), (size_t)G * sizeof(int32_t));
    if (status_out) std::memcpy(status_out, status.data(), (size_t)N * sizeof(int32_t));
    return CUDE_OK;
}

}  // extern "C"
