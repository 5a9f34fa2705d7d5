// libcude_hip.so -- the Metropolis driver (cude_mh_estep, cude_mh_chain): plain, fused into the time-split forward launch,
// the blend step's three states in one launch, and speculative rounds of several steps per dependent launch chain.  The
// depth rules are cude_select.hip's, the candidates' forward launch is cude_launch.hip's forward_sets.
#include "cude_ctx.h"

using namespace cude::api;

namespace {
// How cude_mh_chain speculates (MhSpecArgs, cude_kernels.h): `depth` steps per dependent launch chain -- the candidate
// states those steps can reach as parameter sets of ONE forward launch, then the resolver of the decisions behind their SSEs.
struct SpecRounds {
    int depth = 0;                      // < 2: no speculation
    bool blend = false;                 // gamma < 1 (MhSpecArgs::blend)
    bool split = false;                 // the candidates' forward launch is time-split
    bool resolve_in_scan = false;       // ... and its scan launch, which then holds a subject's candidates in one workgroup,
                                        // resolves the round; otherwise a launch_mh_spec of its own does
    int sets(int d) const { return (blend ? 2 : 1) * ((1 << d) - 1); }
};

// The n_mc steps of the chain in rounds of p.depth.  z / u: the caller's draws on the device (null: the context's
// generator); states: where the chain state after every step goes, or null; cand: sets(depth) rows of N; fwd: the forward
// launch of the candidates (at `cand`, SSEs to fwd.sse), its n_sets filled in here round by round.
int32_t mh_spec_rounds(cude_ctx* c, const SpecRounds& p, const cude::MhArgs& m, double proposal_std, int n_mc,
                       const double* z, const double* u, double* states, double* cand, SetsForward fwd) {
    int32_t rc = CUDE_OK;
    const int64_t N = c->N;
    cude::MhSpecArgs sa{};
    sa.mh = m;
    sa.mh.key = cude::RngKey{c->rng_seed, c->rng_offset, 0};
    sa.blend = p.blend ? 1 : 0;
    sa.cand = cand; sa.sse_sets = fwd.sse; sa.proposal_std = proposal_std;
    sa.depth_resolve = 0; sa.depth_next = std::min(p.depth, n_mc);
    sa.step_resolve = sa.step_next = c->rng_step;
    sa.z_rows = z;
    HIP_TRY(cude::launch_mh_spec(sa, c->stream));                 // the first round's candidates
    int round = 0;
    for (int k = 0; k < n_mc; round++) {
        const int d = std::min(p.depth, n_mc - k);
        sa.depth_resolve = d;
        sa.depth_next = std::min(p.depth, n_mc - k - d);
        sa.step_resolve = c->rng_step + k;
        sa.step_next = c->rng_step + k + d;
        sa.u_rows = u ? u + (size_t)k * N : nullptr;
        sa.z_rows = z ? z + (size_t)(k + d) * N : nullptr;
        // (caller's draws + samples: the states of steps k .. k+d-1 overwrite the normals of those steps, which the
        //  PREVIOUS resolver consumed; the next round's normals are rows k+d ...)
        sa.samples = states ? states + (size_t)k * N : nullptr;
        fwd.n_sets = p.sets(d);
        fwd.resolve_in_scan = p.resolve_in_scan ? &sa : nullptr;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        // kernel timing: every 4th round, and only where the forward launch is the whole round
        if (p.resolve_in_scan && c->timing && round % 4 == 0 && (rc = timed_pair(c, &e0, &e1))) return rc;
        if ((rc = forward_sets(c, fwd))) return rc;
        if (e1) HIP_TRY(hipEventRecord(e1, c->stream));
        if (!p.resolve_in_scan) HIP_TRY(cude::launch_mh_spec(sa, c->stream));
        k += d;
    }
    return CUDE_OK;
}
}  // namespace

extern "C" {

int32_t cude_mh_estep(cude_ctx* c, int32_t n_mc, const double* normals, const double* uniforms, double sigma,
                      double prior_mean, double prior_sd, double proposal_std, double temperature, double gamma,
                      int64_t* accepted) {
    return cude_mh_chain(c, n_mc, normals, uniforms, sigma, prior_mean, prior_sd, proposal_std, temperature, gamma,
                         accepted, nullptr);
}

int32_t cude_mh_chain(cude_ctx* c, int32_t n_mc, const double* normals, const double* uniforms, double sigma,
                      double prior_mean, double prior_sd, double proposal_std, double temperature, double gamma,
                      int64_t* accepted, double* samples) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if (!c->have_pop || !c->have_nn || !c->have_cond) return fail(CUDE_ERR_STATE, "population / parameters not set");
    if (n_mc < 1) return fail(CUDE_ERR_ARG, "n_mc must be >= 1");
    if ((normals == nullptr) != (uniforms == nullptr)) return fail(CUDE_ERR_ARG, "pass both draw arrays or neither");
    const bool device_rng = normals == nullptr;     // draws from the context's counter-based generator (cude_set_rng)
    if (!(sigma > 0) || !(prior_sd > 0) || !(temperature > 0)) return fail(CUDE_ERR_ARG, "sigma, prior_sd, temperature must be > 0");
    const int64_t N = c->N;
    DevBuf<double> d_z, d_u, d_prop, d_sn, d_sc;
    DevBuf<int64_t> d_acc;
    if (!device_rng || samples) HIP_TRY(d_z.resize((size_t)n_mc * N));     // draws, then (samples) the chain states
    if (!device_rng) HIP_TRY(d_u.resize((size_t)n_mc * N));
    HIP_TRY(d_prop.resize(N)); HIP_TRY(d_sn.resize(N)); HIP_TRY(d_sc.resize(N)); HIP_TRY(d_acc.resize(N));
    if (!device_rng) {
        HIP_TRY(push(c, d_z.p, normals, (size_t)n_mc * N));
        HIP_TRY(push(c, d_u.p, uniforms, (size_t)n_mc * N));
    }
    HIP_TRY(hipMemsetAsync(d_acc.p, 0, N * sizeof(int64_t), c->stream));
    cude::MhArgs m{};
    m.N = N; m.p = c->cond.p; m.prop = d_prop.p; m.sse_new = d_sn.p; m.sse_cur = d_sc.p; m.accepted = d_acc.p;
    m.prior_mean = prior_mean; m.prior_sd = prior_sd;
    m.ll_const = -(c->T / 2.0) * std::log(sigma * sigma);
    m.inv_2s2 = 1.0 / (2.0 * sigma * sigma);
    m.temperature = temperature; m.gamma = gamma;
    // The reference re-evaluates the likelihood of the current state in every step (saem.jl:96-97).  With gamma == 1
    // (its burn-in phase, and posterior sampling) the next state is exactly the accepted proposal or the unchanged
    // current one, and the solve is deterministic, so that value is already known: it is carried over instead of
    // recomputed -- the same bits, half the forward launches.  With gamma < 1 the state is a blend and is re-evaluated.
    m.carry_sse = gamma == 1.0 ? 1 : 0;
    if (m.carry_sse && (rc = run_ensemble(c, false, nullptr, true, c->cond.p, d_sc.p))) return rc;
    // Time-split forward path + carried SSE: the proposal is formed inside the forward chunks and accepted inside the
    // scan (Cpep2Args::mh_fused) -- two launches per Metropolis step instead of four, same bits.
    const bool fused = m.carry_sse && is_cpep(c) && !adaptive(c) && c->chunks > 1 && c->opt.mh_fuse;
    // gamma < 1 (the stochastic-approximation phase): the next state is a blend whose likelihood is not known, so a step
    // needed two solves one after the other (the proposal, then the current state again).  The two possible next states
    // depend on (p, q, gamma) alone: they are solved in the SAME launch as the proposal, as three parameter sets, and the
    // decision picks state and SSE (mh_accept_blend_kernel) -- one solve launch per step, the same chain.
    const bool pair = !m.carry_sse && is_cpep(c) && !c->net.generic() && c->opt.mh_pair;
    // Speculative steps (MhSpecArgs, cude_kernels.h): d steps per dependent launch pair -- forward chunks of the 2^d - 1
    // candidate states as parameter sets of ONE launch, then a scan launch that holds a subject's candidates in one
    // workgroup and resolves the d decisions behind their SSEs -- instead of one pair per step.
    // Pays while the candidates still fit the chip beside each other (a shard of an E-step spread over 8 GPUs).
    SpecRounds sp;
    if (fused) {
        sp.depth = mh_spec_depth(c, n_mc);
        sp.split = sp.resolve_in_scan = true;
    } else if (m.carry_sse && is_cpep(c) && (adaptive(c) || c->chunks <= 1) && !c->net.generic()) {
        sp.depth = mh_spec_depth_one_launch(c, n_mc);
    } else if (pair) {
        sp.blend = true;
        sp.split = !adaptive(c) && c->chunks > 1;
        sp.depth = mh_spec_depth_blend(c, n_mc, sp.split);
    }
    // parameter sets per forward launch: a round's candidates, the three of a blend step, or none (one solve per launch)
    const int max_sets = sp.depth >= 2 ? sp.sets(sp.depth) : (pair ? 3 : 0);
    DevBuf<double> d_cand, d_sse_sets, d_part;
    SetsForward fwd;                                      // one network, the candidate states
    if (max_sets > 0) {
        HIP_TRY(d_cand.resize((size_t)max_sets * N));
        HIP_TRY(d_sse_sets.resize((size_t)max_sets * N));
        if ((rc = reserve_sets_forward(c, max_sets, sp.split, d_part))) return rc;
        fwd.cond = d_cand.p; fwd.nn = c->nn.p; fwd.sse = d_sse_sets.p; fwd.partials = d_part.p; fwd.split = sp.split;
    }
    const double* const z = device_rng ? nullptr : d_z.p;
    const double* const u = d_u.p;                        // (null with device draws)
    if (sp.depth >= 2) {
        if ((rc = mh_spec_rounds(c, sp, m, proposal_std, n_mc, z, u, samples ? d_z.p : nullptr, d_cand.p, fwd))) return rc;
    } else if (pair) {
        if ((rc = run_ensemble(c, false, nullptr, true, c->cond.p, d_sc.p))) return rc;      // SSE of the starting state
        fwd.n_sets = 3;
        for (int k = 0; k < n_mc; k++) {
            m.key = cude::RngKey{c->rng_seed, c->rng_offset, c->rng_step + k};
            HIP_TRY(cude::launch_mh_blend_candidates(N, c->cond.p, z ? z + (size_t)k * N : nullptr, m.key, proposal_std, gamma,
                                                     d_cand.p, c->stream));
            if ((rc = forward_sets(c, fwd))) return rc;
            m.u = u ? u + (size_t)k * N : nullptr;
            HIP_TRY(cude::launch_mh_accept_blend(m, d_cand.p, d_sse_sets.p, c->stream));
            if (samples)
                HIP_TRY(hipMemcpyAsync(d_z.p + (size_t)k * N, c->cond.p, N * sizeof(double), hipMemcpyDeviceToDevice,
                                       c->stream));
        }
    } else {
        for (int k = 0; k < n_mc; k++) {          // everything is queued on the stream; one sync at the end
            m.key = cude::RngKey{c->rng_seed, c->rng_offset, c->rng_step + k};
            m.u = u ? u + (size_t)k * N : nullptr;
            if (fused) {
                m.prop = nullptr; m.sse_new = nullptr;
                cude::CpepArgs a = cpep_args(c);
                a.cond = c->cond.p; a.nn = c->nn.p; a.sse = d_sn.p; a.traj = nullptr; a.auc = c->auc.p;
                a.g_cond = c->g_cond.p; a.partials = c->partials.p;
                cude::Cpep2Args a2 = chunk_args(c, a, /*all_blocks=*/true, /*forward_only=*/true);
                a2.mh_fused = 1;
                a2.mh_z = z ? z + (size_t)k * N : nullptr;
                a2.mh_std = proposal_std;
                a2.mh = m;
                hipEvent_t e0 = nullptr, e1 = nullptr;
                // kernel timing: a pair of events costs ~4.5 us of stream time, 10 % of a Metropolis step at 1e4 subjects, so
                // inside this loop of identical launches every 8th step is timed (cude_kernel_time_ms averages those)
                if (c->timing && k % 8 == 0 && (rc = timed_pair(c, &e0, &e1))) return rc;
                HIP_TRY(cude::launch_cpep2(c->net, c->cfg.n_state, false, a2, c->stream));
                if (e1) HIP_TRY(hipEventRecord(e1, c->stream));
            } else {
                HIP_TRY(cude::launch_mh_propose(N, c->cond.p, z ? z + (size_t)k * N : nullptr, m.key, proposal_std, d_prop.p,
                                                c->stream));
                if ((rc = run_ensemble(c, false, nullptr, true, d_prop.p, d_sn.p))) return rc;
                if (!m.carry_sse && (rc = run_ensemble(c, false, nullptr, true, c->cond.p, d_sc.p))) return rc;
                HIP_TRY(cude::launch_mh_accept(m, c->stream));
            }
            if (samples)       // chain state after step k (the draws of this step are no longer needed: reuse their row)
                HIP_TRY(hipMemcpyAsync(d_z.p + (size_t)k * N, c->cond.p, N * sizeof(double), hipMemcpyDeviceToDevice,
                                       c->stream));
        }
    }
    HIP_TRY(fetch(c, samples, d_z.p, (size_t)n_mc * N));
    HIP_TRY(fetch(c, accepted, d_acc.p, N));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (device_rng) c->rng_step += n_mc;            // the next call continues the stream
    return CUDE_OK;
}

}  // extern "C"
