// libcude_hip.so -- the launches: the argument blocks of the context's model, the gradient tape, the ensemble launch of a
// loss / gradient evaluation with the second-stage reductions behind it, parameter sets side by side (gradients:
// eval_sets_device, forward solves: forward_sets), the tangent-linear solve, dense output -- and the entry points that are
// one such launch.  WHICH kernels a launch runs on is cude_select.hip's; the entry points that batch launches are
// cude_batch.hip's and cude_mh.hip's.
#include "cude_ctx.h"

namespace cude {
namespace api {

// population, tables and solver settings of a c-peptide launch; the caller adds parameters and outputs
cude::CpepArgs cpep_args(const cude_ctx* c) {
    cude::CpepArgs a{};
    a.cond_raw = c->cfg.cond_space == CUDE_COND_RAW;
    a.N = c->N;
    a.k0 = c->k0.p; a.k1 = c->k1.p; a.k2 = c->k2.p; a.c0 = c->c0.p;
    a.dG = c->dG.p; a.obs = c->obs.p; a.age = c->age.p;
    a.seg = c->seg.p; a.phi = c->phi.p; a.obs_step = c->obs_step.p; a.obs_w = c->obs_w.p;
    a.stepk = c->stepk.p; a.stepd = c->stepd.p;
    a.T = c->T; a.S = c->cfg.n_steps; a.h = step_size(c); a.inv_n = 1.0 / c->n_global;
    a.tp = c->tp_dev.p; a.TG = c->T; a.out_times = c->tp_dev.p;
    a.t_begin = c->tp.front(); a.t_end = c->tp.back();
    a.abstol = c->abstol; a.reltol = c->reltol;
    a.tape = c->tape.p; a.tape_cap = c->tape_cap; a.tape_n = c->tape_n.p;
    a.gen_acc = c->gen_acc.p;
    a.team = c->opt.adaptive_team ? 0 : -1;
    a.lean_clamp = c->opt.lean_clamp != 0 ? 1 : 0;      // (the kernel decides per wave; any value but 0 is the rule)
    a.perm = (adaptive(c) && !c->slot_of.empty()) ? c->perm.p : nullptr;
    return a;
}

cude::SuppArgs supp_args(const cude_ctx* c) {
    cude::SuppArgs a{};
    a.ckpt_steps_only = (supp_steps_only(c) && !c->net.general()) ? 1 : 0;
    a.N = c->N;
    a.data = c->data.p;
    a.obs_step = c->obs_step.p; a.obs_w = c->obs_w.p;
    a.rho = c->supp_rho.p; a.obs_rho = c->supp_obs_rho.p;
    a.T = c->T; a.S = c->cfg.n_steps; a.h = step_size(c); a.inv_n = 1.0 / c->n_global;
    for (int s = 0; s < 3; s++) a.iscale2[s] = 1.0 / (c->scale[s] * c->scale[s]);
    a.out_times = c->tp_dev.p;
    a.t_begin = c->tp.front(); a.t_end = c->tp.back();
    a.abstol = c->abstol; a.reltol = c->reltol;
    a.tape = c->tape.p; a.tape_cap = c->tape_cap; a.tape_n = c->tape_n.p;
    a.gen_acc = c->gen_acc.p;
    a.perm = (adaptive(c) && !c->slot_of.empty()) ? c->perm.p : nullptr;
    return a;
}

// Tape of the adaptive gradient: per accepted step and subject the step size (c-peptide models: 8 B) or (t, dt, y) and the
// inputs of stages 2..7 (the suppression model: 136 B), + T saved outputs / 2 T residual derivatives.  The reference's
// problems take 10-40 steps at its tolerances; the capacity is what ~4 GB hold, between 64 and 1024 steps
// (option "tape_steps" overrides).  A subject with more accepted steps fails its gradient evaluation (+Inf), not the
// process.  Allocated by the first gradient evaluation (forward-only users of the adaptive mode never pay for it), never
// under stream capture.
// The fallback kernel of a general network (cude_generic.hip) keeps (t_n, dt_n, y_n) of EVERY step -- in the fixed-step
// mode too -- and a lane's P gradient accumulators in HBM: both are allocated here as well.
int generic_tape_rows(const cude_ctx* c) { return 2 + (c->cfg.model == CUDE_MODEL_SUPP ? 3 : c->cfg.n_state); }

int64_t tape_doubles_per_set(const cude_ctx* c) {        // (after ensure_tape)
    if (c->net.generic()) return (int64_t)(adaptive(c) ? c->tape_cap : c->cfg.n_steps) * generic_tape_rows(c) * c->N;
    const int n_state = c->cfg.model == CUDE_MODEL_SUPP ? 3 : 2;
    return adaptive(c) ? cude::adaptive_tape_rows(n_state, c->tape_cap, c->T) * c->N : 0;
}

namespace {
// steps the tape holds at `rows` doubles per step and subject
int tape_capacity(const cude_ctx* c, int rows) {
    int64_t cap = (int64_t)(4e9 / (8.0 * rows * (double)c->N));
    cap = std::max<int64_t>(64, std::min<int64_t>(1024, cap));
    if (c->opt.tape_steps > 0) cap = c->opt.tape_steps;
    return (int)cap;
}
}  // namespace

int32_t ensure_tape(cude_ctx* c) {
    if (c->net.generic()) {
        if (c->tape.p && c->gen_acc.p) return CUDE_OK;
        if (c->capturing) return fail(CUDE_ERR_STATE, "gradient scratch of the general network not allocated before stream capture");
        c->tape_cap = tape_capacity(c, generic_tape_rows(c));
        HIP_TRY(c->tape.resize((size_t)tape_doubles_per_set(c)));
        HIP_TRY(c->gen_acc.resize((size_t)c->P * c->N));
        return CUDE_OK;
    }
    if (!adaptive(c) || c->tape.p) return CUDE_OK;
    if (c->capturing) return fail(CUDE_ERR_STATE, "adaptive gradient tape not allocated before stream capture");
    const int n_state = c->cfg.model == CUDE_MODEL_SUPP ? 3 : 2;
    c->tape_cap = tape_capacity(c, cude::adaptive_tape_rows(n_state));
    HIP_TRY(c->tape.resize((size_t)cude::adaptive_tape_rows(n_state, c->tape_cap, c->T) * c->N));
    return CUDE_OK;
}

// all_blocks: the time-split kernels for every workgroup (forward-only launches, also when the gradient launch is mixed:
// the chunk tables cover all subjects); otherwise from the mixed launch's first time-split block on
cude::Cpep2Args chunk_args(cude_ctx* c, const cude::CpepArgs& base, bool all_blocks, bool forward_only) {
    cude::Cpep2Args a2{};
    a2.base = base;
    a2.L = c->chunks;
    a2.chunk_start = c->chunk_start.p;
    a2.hom_M = c->hom_M.p; a2.hom_obs = c->hom_obs.p; a2.fsum = c->fsum.p; a2.wts = c->res.p;
    if (forward_only && all_blocks && c->chunks_f > 1) {     // the forward-only split and its own transfer matrices
        a2.L = c->chunks_f;
        a2.chunk_start = c->chunk_start_f.p;
        a2.hom_M = c->hom_M_f.p; a2.hom_obs = c->hom_obs_f.p; a2.fsum = c->fsum_f.p; a2.wts = nullptr;
    }
    a2.g_cond_part = c->g_cond_part.p; a2.partials2 = c->partials2.p;
    a2.adj_map = (c->opt.scan_map && !forward_only) ? c->adj_map.p : nullptr;
    a2.scan_bulk_blocks = c->opt.scan_bulk ? c->n_cu : 0;          // (one workgroup per compute unit: its LDS is the scan's)
    a2.base.blk0 = all_blocks ? 0 : c->blk0; a2.base.blk_count = 0;
    return a2;
}

// Kernel timing: a pair of events from the context's pool (grown on demand), the first one recorded on the stream; the
// caller records *e1 behind what it times.  WHICH launches are timed is the caller's rule.
int32_t timed_pair(cude_ctx* c, hipEvent_t* e0, hipEvent_t* e1) {
    if (c->ev_used == c->ev_pool.size()) {
        hipEvent_t a, b;
        HIP_TRY(hipEventCreate(&a));
        HIP_TRY(hipEventCreate(&b));
        c->ev_pool.emplace_back(a, b);
    }
    *e0 = c->ev_pool[c->ev_used].first;
    *e1 = c->ev_pool[c->ev_used].second;
    c->ev_used++;
    HIP_TRY(hipEventRecord(*e0, c->stream));
    return CUDE_OK;
}

namespace {
// Tail of a time-split gradient launch in one launch (launch_chunked_tail): the network gradient over the reverse chunks'
// rows `partials2`, the loss / failure columns over the scan's rows `partials`, and the chunks' shares `g_cond_part` of
// the conditional gradient summed into g_cond (set k at g_cond + k * g_cond_set_stride).  The caller adds what only a
// single-set evaluation has (state advance, page-locked pair, exchange).
cude::ChunkedTailArgs chunked_tail_args(const cude_ctx* c, const double* partials2, const double* partials, double* out,
                                        const double* g_cond_part, double* g_cond, int64_t g_cond_set_stride) {
    cude::ChunkedTailArgs ta{};
    ta.partials2 = partials2; ta.rows2 = c->nblocks * c->chunks;
    ta.partials = partials; ta.rows = c->nblocks;
    ta.P = c->P; ta.out = out; ta.out_stride = c->P + 2;
    ta.mask = c->param_mask.p; ta.n_mask = c->P;
    ta.g_cond_part = g_cond_part; ta.L = c->chunks; ta.N = c->N; ta.g_cond = g_cond; ta.g_cond_set_stride = g_cond_set_stride;
    return ta;
}
}  // namespace

// launches the ensemble kernel + second-stage reduction (+ all-reduce, + L2 term)
// cond_ov / sse_ov: evaluate at other conditional parameters / write the per-subject SSE elsewhere and stop
// after the ensemble kernels (used by the Metropolis E-step, which needs neither loss nor gradient).
int32_t run_ensemble(cude_ctx* c, bool grad, double* traj_dev, bool local_only, const double* cond_ov, double* sse_ov) {
    const bool watch = c->allow_watch;      // (consumed here, before any early return: it belongs to THIS call only)
    c->allow_watch = false;
    if (!c->have_pop) return fail(CUDE_ERR_STATE, "population not set");
    if (!c->have_nn || (!c->have_cond && !cond_ov)) return fail(CUDE_ERR_STATE, "parameters not set");
    if (grad) { int32_t rc = ensure_tape(c); if (rc) return rc; }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool fused_final = false;
    c->loss_in_pinned = false;
    if (c->timing && !c->capturing && (c->timing_count++ % c->timing_period) == 0) {
        int32_t rc = timed_pair(c, &e0, &e1);
        if (rc) return rc;
    }
    if (is_cpep(c)) {
        cude::CpepArgs a = cpep_args(c);
#ifdef CUDE_WAVE_TIMING
        if (grad) {
            HIP_TRY(c->dbg.resize((size_t)c->nblocks * 4));
            a.dbg = c->dbg.p;
        }
#endif
        a.cond = cond_ov ? cond_ov : c->cond.p; a.nn = c->nn.p;
        a.sse = sse_ov ? sse_ov : c->sse.p; a.traj = traj_dev; a.auc = c->auc.p;
        a.g_cond = c->g_cond.p; a.partials = c->partials.p;
        // allocated by cude_set_population_cpep (never here: this function also runs under stream capture)
        if (grad && !adaptive(c) && c->act.p && cpep_act_doubles(c) > 0 && c->act.n >= cpep_act_doubles(c)) {
            a.act = c->act.p;
            a.keep_mode = cpep_keep_mode(c);
        }
        if (c->chunks > 1 && c->blk0 > 0 && grad) {
            // whole rounds: one lane per subject; the remainder: time-split, on a second stream so that its short waves
            // fill the SIMDs the long ones leave one by one (fork / join by events: capturable)
            hipStream_t s2 = c->stream2 ? c->stream2 : c->stream;
            if (c->stream2) {
                HIP_TRY(hipEventRecord(c->ev_fork, c->stream));
                HIP_TRY(hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
            }
            a.blk_count = c->blk0;          // (no alternating issue priority here: it starves the short waves -- measured)
            HIP_TRY(cude::launch_cpep(c->net, c->cfg.n_state, true, a, c->stream));
            a.blk_count = 0;
            cude::Cpep2Args a2 = chunk_args(c, a);
            HIP_TRY(cude::launch_cpep2(c->net, c->cfg.n_state, true, a2, s2));
            if (c->stream2) {
                HIP_TRY(hipEventRecord(c->ev_join, c->stream2));
                HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_join, 0));
            }
        } else if (c->chunks > 1 && (grad || traj_dev == nullptr)) {
            cude::Cpep2Args a2 = chunk_args(c, a, /*all_blocks=*/true, /*forward_only=*/!grad);
            // forward-only on one rank without an L2 term: the scan kernel's workgroups write their (sum SSE, failures)
            // pairs straight into page-locked host memory, which finish_loss adds up (no reduction launch, no copy)
            if (!grad && !sse_ov && !distributed(c) && c->cfg.lambda == 0.0 && c->pinned_pairs &&
                c->pinned_pairs_n >= c->nblocks && !c->capturing && c->opt.fused_final) {
                a2.final_host = c->pinned_pairs;
                fused_final = true;
                // the host watches the pairs arrive (finish_loss) instead of going through the runtime's completion wait
                // (forward call at 1e4 subjects 56.9 -> 51.6 us, at 57 subjects 41.3 -> 36.6 us): every slot starts as a
                // NaN no kernel produces.  Option "poll_pinned" = 0 (CUDE_NO_POLL_PINNED=1): plain hipStreamSynchronize.
                c->poll_pairs = c->opt.poll_pinned && c->poll_ok && watch;
                if (c->poll_pairs) {
                    volatile uint64_t* w = reinterpret_cast<volatile uint64_t*>(c->pinned_pairs);
                    for (int64_t q = 0; q < 2 * c->nblocks; q++) w[q] = kPairSentinel;
                }
            }
            a2.defer_chunk_sum = grad && c->blk0 == 0 && c->opt.fused_tail;      // (summed by the one tail launch below)
            HIP_TRY(cude::launch_cpep2(c->net, c->cfg.n_state, grad, a2, c->stream));
        } else {
            if (grad && !adaptive(c)) {
                a.prio_shift = prio_shift_for(c, c->nblocks);
                a.prio_clock = a.prio_shift > 0 ? prio_clock_for(c) : 0;
            }
            if (grad && adaptive(c)) {      // adaptive gradient kernel: at most two waves per SIMD (measured -4.8 %)
                a.prio_shift = c->opt.prio_shift >= 0
                                   ? c->opt.prio_shift
                                   : ((c->nblocks > c->half_slots && c->nblocks <= 2 * c->half_slots) ? 5 : 0);
            }
            HIP_TRY(cude::launch_cpep(c->net, c->cfg.n_state, grad, a, c->stream));
        }
    } else {
        cude::SuppArgs a = supp_args(c);
        a.cond = cond_ov ? cond_ov : c->cond.p; a.nn = c->nn.p;
        a.ckpt = c->ckpt.p; a.sse = sse_ov ? sse_ov : c->sse.p; a.traj = traj_dev;
        // allocated by cude_set_population_supp (never here: this function also runs under stream capture)
        if (grad && !a.ckpt_steps_only && c->act.p && c->act.n >= supp_act_doubles(c)) a.act = c->act.p;
        a.g_cond = c->g_cond.p; a.partials = c->partials.p;
        HIP_TRY(cude::launch_supp(c->net, grad, a, c->stream));
    }
    if (e1) HIP_TRY(hipEventRecord(e1, c->stream));
    note_adaptive_launch(c, grad);          // (a forward launch overwrites the counts cude_adaptive_steps pairs the tape with)
    if (sse_ov) return CUDE_OK;
    const int P = c->P;
    const bool fold = c->fold_advance && grad && !local_only;
    // who sums over the ranks: the reduction kernels themselves through the peer-write exchange (no further launch; the
    // pair [sum loss, n_failed] they leave is already global), or an RCCL all-reduce behind them
    const bool xc = c->xchg.ready && !local_only;
    const bool rccl = !xc && c->comm != nullptr && !local_only;
    const cude::XchgArgs xargs = xc ? xchg_args(c) : cude::XchgArgs{};
    const cude::XchgArgs* xq = xc ? &xargs : nullptr;
    const cude::TailAdvance adv_args = tail_advance(c);
    const cude::TailAdvance* adv_red = (fold && !rccl && c->cfg.lambda == 0.0) ? &adv_args : nullptr;
    const cude::TailAdvance* adv_l2 = (fold && c->cfg.lambda != 0.0) ? &adv_args : nullptr;
    c->advance_done = adv_red != nullptr || adv_l2 != nullptr;
    // no L2 term, no RCCL call behind, not capturing: the reduction that finishes [sum loss, n_failed] writes the pair into
    // the page-locked result buffer too, and finish_loss watches it arrive instead of queueing a copy and waiting for the stream
    double* host_tail = nullptr;
    {
        // (not with the exchange: a wait that gave up is reported through the status word, read after the stream's end)
        if (c->opt.poll_pinned && c->poll_ok && watch && c->pinned && !rccl && !xc && c->cfg.lambda == 0.0 && !c->capturing &&
            !local_only && !fused_final) {
            host_tail = c->pinned + P;
            volatile uint64_t* w = reinterpret_cast<volatile uint64_t*>(host_tail);
            w[0] = kPairSentinel; w[1] = kPairSentinel;
        }
        c->tail_in_pinned = host_tail != nullptr;
    }
    if (grad && is_cpep(c) && c->chunks > 1 && c->blk0 > 0) {
        HIP_TRY(cude::launch_reduce_cols(c->partials.p, c->blk0, P + 2, 0, P, c->g_nn.p, c->stream, 1, c->param_mask.p, P));
        HIP_TRY(cude::launch_reduce_cols(c->partials2.p, (c->nblocks - c->blk0) * c->chunks, P, 0, P, c->g_nn.p, c->stream, 1,
                                         c->param_mask.p, P, 0, /*accumulate=*/true, nullptr, nullptr, xq));
        HIP_TRY(cude::launch_reduce_cols(c->partials.p, c->nblocks, P + 2, P, 2, c->g_nn.p, c->stream, 1, nullptr, 0, 0, false,
                                         adv_red, host_tail, xq));
    } else if (grad && is_cpep(c) && c->chunks > 1 && c->opt.fused_tail) {
        // one launch: the network gradient over the reverse chunks' rows, the loss / failure columns over the scan's rows
        // (+ state advance, page-locked pair, exchange) and the chunks' shares of the conditional gradient
        cude::ChunkedTailArgs ta =
            chunked_tail_args(c, c->partials2.p, c->partials.p, c->g_nn.p, c->g_cond_part.p, c->g_cond.p, c->N);
        if (adv_red) ta.adv = *adv_red;
        ta.host_tail = host_tail;
        if (xq) ta.xchg = *xq;
        HIP_TRY(cude::launch_chunked_tail(ta, 1, c->stream));
    } else if (grad && is_cpep(c) && c->chunks > 1) {
        HIP_TRY(cude::launch_reduce_cols(c->partials2.p, c->nblocks * c->chunks, P, 0, P, c->g_nn.p, c->stream, 1,
                                         c->param_mask.p, P, 0, false, nullptr, nullptr, xq));
        HIP_TRY(cude::launch_reduce_cols(c->partials.p, c->nblocks, P + 2, P, 2, c->g_nn.p, c->stream, 1, nullptr, 0, 0, false,
                                         adv_red, host_tail, xq));
    } else if (grad) {
        HIP_TRY(cude::launch_reduce_cols(c->partials.p, c->nblocks, P + 2, 0, P + 2, c->g_nn.p, c->stream, 1,
                                         c->param_mask.p, P, 0, false, adv_red, host_tail, xq));
    } else if (fused_final) {
        c->loss_in_pinned = true;
    } else {
        HIP_TRY(cude::launch_reduce_cols(c->partials.p, c->nblocks, P + 2, P, 2, c->g_nn.p, c->stream, 1, nullptr, 0, 0, false,
                                         nullptr, host_tail, xq));
    }
    if (local_only) return CUDE_OK;   // the caller reduces across ranks and applies the L2 term
    if (rccl) {
        int32_t rc = grad ? allreduce_dev(c, c->g_nn.p, P + 2) : allreduce_dev(c, c->g_nn.p + P, 2);
        if (rc) return rc;
    }
    if (c->cfg.lambda != 0.0) {
        if (!grad) HIP_TRY(hipMemsetAsync(c->g_nn.p, 0, P * sizeof(double), c->stream));
        HIP_TRY(cude::launch_l2_term(c->nn.p, P, c->cfg.lambda, c->n_global, c->g_nn.p, c->stream, c->param_mask.p, adv_l2));
    }
    return CUDE_OK;
}

// copies [loss_sum, n_failed] (and optionally g_nn) back and forms the reference's loss value
int32_t finish_loss(cude_ctx* c, double* loss, double* g_nn_host) {
    const int P = c->P;
    std::vector<double> pageable;
    if (!c->pinned) pageable.resize(P + 2);
    double* const tmp = c->pinned ? c->pinned : pageable.data();      // page-locked: no staging copy behind the sync
    const bool watch_tail = c->tail_in_pinned && !g_nn_host && !c->loss_in_pinned && c->pinned;
    c->tail_in_pinned = false;
    if (g_nn_host) {
        HIP_TRY(fetch(c, tmp, c->g_nn.p, P + 2));
    } else if (!c->loss_in_pinned && !watch_tail) {
        HIP_TRY(fetch(c, tmp + P, c->g_nn.p + P, 2));
    }
    bool arrived = false, watch_timed_out = false;
    if (watch_tail) {
        volatile uint64_t* w = reinterpret_cast<volatile uint64_t*>(c->pinned + P);
        const auto t0 = std::chrono::steady_clock::now();
        for (int spin = 0; !arrived; spin++) {
            arrived = w[0] != kPairSentinel && w[1] != kPairSentinel;
            if (!arrived && (spin & 63) == 63 &&
                std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        if (!arrived) {     // (a kernel that never got there: let the ordinary path report it / fetch the pair)
            HIP_TRY(fetch(c, tmp + P, c->g_nn.p + P, 2));
            watch_timed_out = true;
        }
    }
    if (c->loss_in_pinned && !g_nn_host && c->poll_pairs) {
        // the pairs are written into page-locked host memory by the last kernel of the call: watching them arrive skips
        // the runtime's completion path; bounded (a faulting kernel never writes them): then the ordinary wait decides
        volatile uint64_t* w = reinterpret_cast<volatile uint64_t*>(c->pinned_pairs);
        const auto t0 = std::chrono::steady_clock::now();
        for (int spin = 0; !arrived; spin++) {
            arrived = true;
            for (int64_t q = 2 * c->nblocks - 1; q >= 0; q--)
                if (w[q] == kPairSentinel) { arrived = false; break; }
            if (!arrived && (spin & 63) == 63 &&
                std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(5)) break;
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        watch_timed_out = !arrived;
    }
    c->poll_pairs = false;
    if (!arrived) HIP_TRY(hipStreamSynchronize(c->stream));
    if (watch_timed_out && !distributed(c)) {
        // Either this launch takes longer than the watch's limit (then the few microseconds a watch saves do not matter to
        // it) or device stores to this host memory do not become visible while a kernel runs (a non-coherent mapping:
        // every later watch would burn its whole limit): in both cases this context goes back to plain stream waits.
        c->poll_ok = false;
        if (c->opt.debug_selector)
            fprintf(stderr, "[cude] a watched result did not arrive within its time limit: plain stream waits from now on\n");
    }
    if (c->loss_in_pinned && !g_nn_host) {
        // the scan kernel's per-workgroup pairs, added in the order of reduce_partials_kernel (256 strided partial sums,
        // then the halving tree), so that the value does not depend on which of the two ways produced it
        for (int col = 0; col < 2; col++) {
            double part[256];
            for (int t = 0; t < 256; t++) {
                double v = 0.0;
                for (int64_t b = t; b < c->nblocks; b += 256) v += c->pinned_pairs[2 * b + col];
                part[t] = v;
            }
            for (int off = 128; off >= 1; off >>= 1)
                for (int t = 0; t < off; t++) part[t] += part[t + off];
            tmp[P + col] = part[0];
        }
    }
    c->loss_in_pinned = false;
    if (c->xchg.ready) {        // a wait of the exchange that ran out of time (in ANY column, not only the loss's)
        if (arrived) HIP_TRY(hipStreamSynchronize(c->stream));
        const int32_t xrc = xchg_check(c);
        if (xrc) return xrc;
    }
    c->last_failed = (int64_t)std::llround(tmp[P + 1]);
    if (g_nn_host) std::memcpy(g_nn_host, tmp, P * sizeof(double));
    if (loss) *loss = (c->last_failed > 0 || !std::isfinite(tmp[P])) ? std::numeric_limits<double>::infinity()
                                                                     : tmp[P] / c->n_global;
    return CUDE_OK;
}

// (see cude_adaptive_regroup in include/cude.h)
// Entry points that launch a large adaptive population again and again (restarts trained side by side, per-subject
// fits) keep the launch ordered by accepted-step count as cude_adam_run does: once the counts of a first evaluation are
// there, then after every kRegroupEvals-th evaluation they make (the counts drift with the parameters).  Per-subject
// results do not depend on the order; the shared gradient's summation order does (rounding).
int32_t maybe_regroup(cude_ctx* c) {
    constexpr int64_t kRegroupEvals = 200;
    if (!adaptive(c) || c->N < 8192 || !c->opt.auto_regroup || !c->have_counts || c->capturing || c->net.generic()) return CUDE_OK;
    if (!c->slot_of.empty() && c->evals_since_regroup < kRegroupEvals) { c->evals_since_regroup++; return CUDE_OK; }
    return adaptive_regroup(c, nullptr, nullptr);
}

int32_t adaptive_regroup(cude_ctx* c, int32_t* spread_before, int32_t* spread_after) {
    if (c->net.generic()) return fail(CUDE_ERR_UNSUPPORTED, "the fallback kernel of a general network runs in the caller's order");
    if (!adaptive(c) || !c->have_counts) return fail(CUDE_ERR_STATE, "no adaptive evaluation on this context yet");
    const int64_t N = c->N;
    std::vector<int32_t> n_acc((size_t)N);
    HIP_TRY(fetch(c, n_acc.data(), c->tape_n.p, N));
    HIP_TRY(hipStreamSynchronize(c->stream));
    // mean over the waves of (largest - smallest accepted-step count among the wave's lanes), in the current order
    auto spread = [&](const std::vector<int32_t>& order) {
        int64_t tot = 0, waves = 0;
        for (int64_t b = 0; b < N; b += cude::kBlock) {
            int32_t lo = INT32_MAX, hi = 0;
            for (int64_t k = b; k < std::min<int64_t>(b + cude::kBlock, N); k++) {
                const int32_t v = n_acc[(size_t)(order.empty() ? k : order[(size_t)k])];
                lo = std::min(lo, v); hi = std::max(hi, v);
            }
            tot += hi - lo; waves++;
        }
        return (int32_t)((tot + waves / 2) / std::max<int64_t>(waves, 1));
    };
    std::vector<int32_t> cur;
    if (!c->slot_of.empty()) {
        cur.resize((size_t)N);
        for (int64_t sbj = 0; sbj < N; sbj++) cur[(size_t)c->slot_of[(size_t)sbj]] = (int32_t)sbj;
    }
    if (spread_before) *spread_before = spread(cur);
    std::vector<int32_t> order((size_t)N);
    for (int64_t k = 0; k < N; k++) order[(size_t)k] = (int32_t)k;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return n_acc[(size_t)x] > n_acc[(size_t)y]; });
    if (spread_after) *spread_after = spread(order);
    if (c->slot_of.empty() || c->perm.n != (size_t)N) drop_graph(c);   // the launches' `perm` argument changes (null -> buffer)
    HIP_TRY(c->perm.resize((size_t)N));
    HIP_TRY(push(c, c->perm.p, order.data(), N));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->slot_of.assign((size_t)N, 0);
    for (int64_t k = 0; k < N; k++) c->slot_of[(size_t)order[(size_t)k]] = (int32_t)k;
    c->have_tape = false;                           // the tape on the device is in the OLD launch order
    c->evals_since_regroup = 0;
    return CUDE_OK;
}

// Loss sums and gradients of n_sets parameter sets that are ALREADY on the device (set k: nn + k * stride_nn,
// cond + k * stride_cond), everything queued on the context's stream, no synchronisation, no host copy:
//   g_cond + k * stride_cond   <- dL/dcond of set k                               [N]
//   out + k * (P + 2)          <- [masked network gradient (P); sum of SSE; failed subjects], summed over the ranks
// (the L2 term and the loss value are the caller's: launch_finish_sets).  The set index is the grid's second dimension
// (third on the time-split path); sets are launched in groups as large as the scratch budget allows.
// rows (cude_subject_scores): the launches also leave every lane's own gradient row and the per-subject SSEs behind, in the
// caller's tables.  Such a call always takes the one-lane kernels, with inv_n = 1 (a row is d SSE_i / d theta itself),
// needs stride_cond == N, and leaves `out` this rank's own (it is the caller's scratch).
int32_t eval_sets_device(cude_ctx* c, int64_t n_sets, const double* nn, int64_t stride_nn, const double* cond,
                         int64_t stride_cond, double* g_cond, double* out, const SetsRows* rows) {
    int32_t rc = CUDE_OK;
    const int P = c->P, S = c->cfg.n_steps;
    const int64_t N = c->N, nb = c->nblocks;
    const bool supp = c->cfg.model == CUDE_MODEL_SUPP;
    // Small populations: K restarts of a few dozen subjects are K single-wave chains on the one-lane kernel (25 waves on
    // 1024 SIMDs, each paying the full single-wave latency).  When the population itself runs time-split (chunks > 1) and
    // the sets do not fill the chip either, the time-split kernels take the set index as a third grid dimension: K x L
    // short waves instead.  Same kernels as cude_loss_grad on this context, so a set's result is bit-identical to it.
    const int L = c->chunks;
    const bool split = !supp && L > 1 && c->blk0 == 0 && nb * (int64_t)std::min<int64_t>(n_sets, 64) <= 512 &&
                       c->opt.ms_split && !rows;
    if (rows && stride_cond != N) return fail(CUDE_ERR_ARG, "gradient rows need the sets' conditionals as [n_sets][N]");
    if ((rc = ensure_tape(c))) return rc;                 // (fixes the capacity the per-set tapes share)
    if ((rc = maybe_regroup(c))) return rc;
    const bool gen = c->net.generic();
    const int64_t tape_rows = tape_doubles_per_set(c) / N;
    const double per_set = 8.0 * ((double)nb * (P + 2) + (double)tape_rows * N + (gen && !rows ? (double)P * N : 0.0) +
                                  (supp && !adaptive(c) ? (double)cude::supp_ckpt_rows(S, c->T) * N : 0.0) +
                                  (split ? (double)L * (3 + c->T) * N + 5.0 * S * N + (double)L * N + (double)L * nb * P : 0.0));
    // sets per launch: bounded by the grid's y / z dimension and the scratch budget
    const int64_t chunk = sets_per_launch(n_sets, split ? 16384 : 32768, sets_scratch_budget(c), per_set);
    if (split) {
        HIP_TRY(c->ms_fsum.reserve((size_t)chunk * L * (3 + c->T) * N));
        HIP_TRY(c->ms_wts.reserve((size_t)chunk * 5 * S * N));
        HIP_TRY(c->ms_gcp.reserve((size_t)chunk * L * N));
        HIP_TRY(c->ms_p2.reserve((size_t)chunk * L * nb * P));
    }
    HIP_TRY(c->ms_part.reserve((size_t)chunk * nb * (P + 2)));
    if (supp && !adaptive(c) && !gen) HIP_TRY(c->ms_ckpt.reserve((size_t)chunk * cude::supp_ckpt_rows(S, c->T) * N));
    if (adaptive(c) || gen) HIP_TRY(c->ms_tape.reserve((size_t)chunk * tape_rows * N));
    if (gen && !rows) HIP_TRY(c->ms_gacc.reserve((size_t)chunk * P * N));
    // (the fallback kernel's accumulators ARE the rows: they go straight into the caller's table)
    const auto want_rows = [&](auto& a, int64_t k0) {
        a.inv_n = 1.0;
        a.sse = rows->sse + k0 * N;
        a.lane_rows = rows->rows + k0 * (int64_t)P * N;
        if (gen) a.gen_acc = a.lane_rows;
        a.unit_seed = rows->unit_seed > 0 ? rows->unit_seed + (int32_t)k0 : 0;
    };
    for (int64_t k0 = 0; k0 < n_sets; k0 += chunk) {
        const int64_t kn = std::min<int64_t>(chunk, n_sets - k0);
        const double* nn_k = nn + k0 * stride_nn;
        const double* cond_k = cond + k0 * stride_cond;
        double* g_cond_k = g_cond + k0 * stride_cond;
        double* out_k = out + k0 * (P + 2);
        if (split) {
            cude::CpepArgs a = cpep_args(c);
            a.cond = cond_k; a.nn = nn_k;
            a.g_cond = g_cond_k; a.partials = c->ms_part.p;
            a.sse = nullptr; a.traj = nullptr; a.auc = nullptr;
            a.n_sets = (int32_t)kn; a.set_stride_nn = stride_nn; a.set_stride_cond = stride_cond;
            cude::Cpep2Args a2 = chunk_args(c, a);
            a2.fsum = c->ms_fsum.p; a2.wts = c->ms_wts.p; a2.g_cond_part = c->ms_gcp.p; a2.partials2 = c->ms_p2.p;
            a2.defer_chunk_sum = c->opt.fused_tail;
            HIP_TRY(cude::launch_cpep2(c->net, c->cfg.n_state, true, a2, c->stream));
            // network gradient: the reverse chunks' partial rows; loss / failure columns: the scan's
            if (c->opt.fused_tail) {
                const cude::ChunkedTailArgs ta =
                    chunked_tail_args(c, c->ms_p2.p, c->ms_part.p, out_k, c->ms_gcp.p, g_cond_k, stride_cond);
                HIP_TRY(cude::launch_chunked_tail(ta, (int)kn, c->stream));
            } else {
                HIP_TRY(cude::launch_reduce_cols(c->ms_p2.p, nb * L, P, 0, P, out_k, c->stream, (int)kn, c->param_mask.p, P, P + 2));
                HIP_TRY(cude::launch_reduce_cols(c->ms_part.p, nb, P + 2, P, 2, out_k, c->stream, (int)kn));
            }
        } else if (!supp) {
            cude::CpepArgs a = cpep_args(c);
            a.cond = cond_k; a.nn = nn_k;
            a.g_cond = g_cond_k; a.partials = c->ms_part.p;
            a.n_sets = (int32_t)kn; a.set_stride_nn = stride_nn; a.set_stride_cond = stride_cond;
            if (adaptive(c) || gen) a.tape = c->ms_tape.p;     // (tape_n: the counts of set 0, for the re-ordering)
            if (gen) a.gen_acc = c->ms_gacc.p;
            if (rows) { want_rows(a, k0); a.team = -1; }
            // (several sets are several rounds: no alternating issue priority by the library's rule; an explicit "prio_shift"
            // option is honoured, so that the switch can be exercised on these launches too)
            if (!adaptive(c) && !gen && c->opt.prio_shift > 0) {
                a.prio_shift = c->opt.prio_shift;
                a.prio_clock = prio_clock_for(c);
            }
            HIP_TRY(cude::launch_cpep(c->net, c->cfg.n_state, true, a, c->stream));     // one-lane kernel: the sets fill the chip
        } else {
            cude::SuppArgs a = supp_args(c);
            a.cond = cond_k; a.nn = nn_k;
            a.ckpt = c->ms_ckpt.p; a.g_cond = g_cond_k; a.partials = c->ms_part.p;
            if (adaptive(c) || gen) a.tape = c->ms_tape.p;
            if (gen) a.gen_acc = c->ms_gacc.p;
            if (rows) { want_rows(a, k0); a.ckpt_steps_only = 0; }      // (the stage-input kernel: the one compiled with rows)
            if (!rows && !adaptive(c) && !a.ckpt_steps_only && supp_keep_activations(c, kn)) {
                HIP_TRY(c->ms_act.reserve((size_t)kn * supp_act_doubles(c)));
                a.act = c->ms_act.p;
            }
            a.n_sets = (int32_t)kn; a.set_stride_nn = stride_nn; a.set_stride_cond = stride_cond;
            HIP_TRY(cude::launch_supp(c->net, true, a, c->stream));
        }
        note_adaptive_launch(c, false);     // (step counts of the first set; its tape is ms_tape)
        if (!split)
            HIP_TRY(cude::launch_reduce_cols(c->ms_part.p, nb, P + 2, 0, P + 2, out_k, c->stream, (int)kn, c->param_mask.p, P));
        if (!rows && distributed(c) && (rc = allreduce_dev(c, out_k, (size_t)kn * (P + 2)))) return rc;
    }
    return CUDE_OK;
}

// Queues one tangent-linear solve of the context's model at `cond` on its stream: the per-subject SSE goes to `sse`, the
// sums of `out` next to it, [sum SSE, failures] to c->partials.  keep_tape = false: an adaptive solve records no steps.
// obs_ov: the residuals are taken against these observations (the population's layout) instead of the population's.
hipError_t launch_tangent(cude_ctx* c, const double* cond, double* sse, const cude::SensOut& out, bool keep_tape,
                          const double* obs_ov) {
    const auto fill = [&](auto& a) {
        a.cond = cond; a.nn = c->nn.p; a.sse = sse; a.partials = c->partials.p;
        if (!keep_tape) a.tape = nullptr;
        a.out = out;
    };
    if (is_cpep(c)) {
        cude::CpepSensArgs a{};
        static_cast<cude::CpepArgs&>(a) = cpep_args(c);
        fill(a);
        if (obs_ov) a.obs = obs_ov;
        return cude::launch_cpep_sens(c->net, c->cfg.n_state, a, c->stream);
    }
    cude::SuppSensArgs a{};
    static_cast<cude::SuppArgs&>(a) = supp_args(c);
    fill(a);
    if (obs_ov) a.data = obs_ov;
    return cude::launch_supp_sens(c->net, a, c->stream);
}

hipError_t launch_tangent2(cude_ctx* c, const double* cond, double* sse, const cude::SensOut& out, const cude::CurvOut& out2,
                           bool keep_tape) {
    const auto fill = [&](auto& a) {
        a.cond = cond; a.nn = c->nn.p; a.sse = sse; a.partials = c->partials.p;
        if (!keep_tape) a.tape = nullptr;
        a.out = out;
        a.out.sens = nullptr;
        a.out2 = out2;
    };
    if (is_cpep(c)) {
        cude::CpepCurvArgs a{};
        static_cast<cude::CpepArgs&>(a) = cpep_args(c);
        fill(a);
        return cude::launch_cpep_curv(c->net, c->cfg.n_state, a, c->stream);
    }
    cude::SuppCurvArgs a{};
    static_cast<cude::SuppArgs&>(a) = supp_args(c);
    fill(a);
    return cude::launch_supp_curv(c->net, a, c->stream);
}

// (SetsForward: cude_ctx.h)
// Scratch of forward_sets for up to max_sets sets per launch.  A split launch works in the context's own (ms_fsum: every
// set's forced chunk responses, ms_part: kept between calls), any other in the caller's `own_part`, which goes into
// SetsForward::partials.  Never under stream capture (no entry point that batches solves runs there).
int32_t reserve_sets_forward(cude_ctx* c, int64_t max_sets, bool split, DevBuf<double>& own_part) {
    const size_t part = (size_t)max_sets * c->nblocks * (c->P + 2);
    if (!split) {
        HIP_TRY(own_part.resize(part));
        return CUDE_OK;
    }
    HIP_TRY(c->ms_fsum.reserve((size_t)max_sets * forward_chunks(c) * (3 + c->T) * c->N));
    HIP_TRY(c->ms_part.reserve(part));
    return CUDE_OK;
}

// Queues the launch on the context's stream; no synchronisation.
int32_t forward_sets(cude_ctx* c, const SetsForward& s) {
    const auto fill = [&](auto& a) {
        a.cond = s.cond; a.nn = s.nn; a.sse = s.sse;
        a.partials = s.split ? c->ms_part.p : s.partials;
        a.n_sets = s.n_sets; a.set_stride_nn = s.stride_nn; a.set_stride_cond = c->N;
    };
    if (!is_cpep(c)) {
        cude::SuppArgs a = supp_args(c);
        fill(a);
        HIP_TRY(cude::launch_supp(c->net, false, a, c->stream));
    } else {
        cude::CpepArgs a = cpep_args(c);
        fill(a);
        if (s.split) {
            cude::Cpep2Args a2 = chunk_args(c, a, /*all_blocks=*/true, /*forward_only=*/true);
            a2.fsum = c->ms_fsum.p;
            if (s.resolve_in_scan) {
                a2.spec_slots = 1 << s.resolve_in_scan->depth_resolve;
                a2.spec = *s.resolve_in_scan;
            }
            HIP_TRY(cude::launch_cpep2(c->net, c->cfg.n_state, false, a2, c->stream));
        } else {
            HIP_TRY(cude::launch_cpep(c->net, c->cfg.n_state, false, a, c->stream));
        }
    }
    note_adaptive_launch(c, false);         // (the counts of set 0 overwrite those a gradient's tape went with)
    return CUDE_OK;
}

// Dense output.  Fixed-step mode: the step every output falls into (as locate_obs: tau in (t_n, t_{n+1}]), its seven
// interpolation weights and, for the suppression model, state 1 at the outputs (the closed form of the launch tables).
// Adaptive mode: the kernel interpolates at the times themselves.
int32_t OutputTables::upload(cude_ctx* c, int64_t n, const double* times) {
    if (adaptive(c)) {
        HIP_TRY(d_times.resize((size_t)n));
        HIP_TRY(push(c, d_times.p, times, n));
        return CUDE_OK;
    }
    const int S = c->cfg.n_steps;
    const double t0 = c->tp.front(), h = (c->tp.back() - t0) / S;
    step.resize((size_t)n);
    w.resize((size_t)n * 7);
    for (int64_t i = 0; i < n; i++) {
        const double x = (times[i] - t0) / h;
        int m = (int)std::ceil(x - 1e-9) - 1;
        m = std::min(std::max(m, 0), S - 1);
        step[(size_t)i] = m;
        interp_weights((times[i] - (t0 + m * h)) / h, &w[(size_t)i * 7]);
    }
    HIP_TRY(d_step.resize((size_t)n));
    HIP_TRY(d_w.resize((size_t)n * 7));
    HIP_TRY(push(c, d_step.p, step.data(), n));
    HIP_TRY(push(c, d_w.p, w.data(), n * 7));
    if (!is_cpep(c)) {
        supp_output_rho(S, h, step, w, rho);
        HIP_TRY(d_rho.resize((size_t)n));
        HIP_TRY(push(c, d_rho.p, rho.data(), n));
    }
    return CUDE_OK;
}

// Queues the outputs-only launch (no residuals, no SSE) on the context's stream; no synchronisation.
int32_t launch_dense(cude_ctx* c, const OutputTables& t, const DenseLaunch& d) {
    const auto fill = [&](auto& a) {
        a.cond = d.cond; a.nn = c->nn.p;
        a.obs_step = t.d_step.p + d.k0; a.obs_w = t.d_w.p + 7 * d.k0; a.out_times = t.d_times.p + d.k0;
        a.T = (int32_t)d.kn;
        a.traj = d.traj; a.partials = d.partials;
        if (!d.keep_perm) a.perm = nullptr;     // (a launch order would take subjects from outside a stretch of workgroups)
        a.n_sets = d.n_sets; a.set_stride_nn = 0; a.set_stride_cond = d.n_sets ? c->N : 0;
        a.traj_set_stride = d.set_stride; a.blk_first = d.blk_first; a.blk_count = d.blk_count;
    };
    if (is_cpep(c)) {
        cude::CpepArgs a = cpep_args(c);
        a.obs = nullptr;
        fill(a);
        HIP_TRY(cude::launch_cpep(c->net, c->cfg.n_state, false, a, c->stream));
    } else {
        cude::SuppArgs a = supp_args(c);
        a.ckpt_steps_only = 0;
        fill(a);
        a.obs_rho = t.d_rho.p + d.k0;
        a.T_data = c->T;                        // outputs only: u0 = the data's first column
        a.traj_ss = d.traj_ss; a.traj_st = d.traj_st; a.traj_sn = d.traj_sn;
        HIP_TRY(cude::launch_supp(c->net, false, a, c->stream));
    }
    note_adaptive_launch(c, false);
    return CUDE_OK;
}

}  // namespace api
}  // namespace cude

using namespace cude::api;

extern "C" {

int32_t cude_forward(cude_ctx* c, double* loss, double* per_subject_sse, double* traj) {
    int32_t rc = bind(c);
    if (rc) return rc;
    double* traj_dev = nullptr;
    if (traj) {
        if (!c->have_pop) return fail(CUDE_ERR_STATE, "population not set");
        HIP_TRY(c->traj.resize((size_t)c->cfg.n_state * c->T * c->N));
        traj_dev = c->traj.p;
    }
    c->allow_watch = !per_subject_sse && !traj;        // (copies into caller memory pending: the stream must be waited for)
    if ((rc = run_ensemble(c, false, traj_dev))) return rc;
    HIP_TRY(fetch(c, per_subject_sse, c->sse.p, c->N));
    HIP_TRY(fetch(c, traj, c->traj.p, c->traj.n));
    return finish_loss(c, loss, nullptr);
}

int32_t cude_loss_grad(cude_ctx* c, double* loss, double* g_nn, double* g_cond) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if ((rc = run_ensemble(c, true, nullptr))) return rc;
    HIP_TRY(fetch(c, g_cond, c->g_cond.p, c->N));
    return finish_loss(c, loss, g_nn);
}

int32_t cude_n_outputs(cude_ctx* c, int32_t* n_out) {
    if (!c || !n_out) return fail(CUDE_ERR_ARG, "null argument");
    if (!c->have_pop) return fail(CUDE_ERR_STATE, "population not set");
    *n_out = is_cpep(c) ? c->T : 3 * c->T;
    return CUDE_OK;
}

int32_t cude_n_failed(cude_ctx* c, int64_t* n_failed) {
    if (!c || !n_failed) return fail(CUDE_ERR_ARG, "null argument");
    *n_failed = c->last_failed;
    return CUDE_OK;
}

int32_t cude_adaptive_regroup(cude_ctx* c, int32_t* spread_before, int32_t* spread_after) {
    int32_t rc = bind(c);
    if (rc) return rc;
    return adaptive_regroup(c, spread_before, spread_after);
}

int32_t cude_adaptive_steps(cude_ctx* c, int64_t subject, int32_t cap, double* t_out, double* dt_out, int32_t* n_steps) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if (!n_steps || cap < 0) return fail(CUDE_ERR_ARG, "null/negative argument");
    if (!adaptive(c) || !c->have_tape) return fail(CUDE_ERR_STATE, "no adaptive gradient evaluation on this context yet");
    if (subject < 0 || subject >= c->N) return fail(CUDE_ERR_ARG, "subject out of range");
    int32_t n = 0;
    HIP_TRY(fetch(c, &n, c->tape_n.p + subject, 1));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *n_steps = n;
    // (the fallback kernel of a general network keeps (t_n, dt_n, y_n) for either model, as the suppression kernels do)
    const bool supp = c->cfg.model == CUDE_MODEL_SUPP || c->net.generic();
    const int rows = c->net.generic() ? generic_tape_rows(c) : cude::adaptive_tape_rows(supp ? 3 : 2);
    const int m = std::min(std::min(n, cap), c->tape_cap);
    const int64_t slot = c->slot_of.empty() ? subject : c->slot_of[(size_t)subject];      // the tape is in launch order
    if (m < 1) return CUDE_OK;
    // entry k, row r of the tape: one double every rows * N.  Suppression model: rows 0 and 1 are (t_n, dt_n); c-peptide
    // models keep dt_n alone and t_n is the forward sweep's own running sum t_{n+1} = t_n + dt_n from the initial time
    // (the same additions in the same order: the same bits)
    std::vector<double> dts;
    double* dt_dst = dt_out;
    if (!supp && !dt_dst) { dts.resize((size_t)m); dt_dst = dts.data(); }
    if (supp && t_out)
        HIP_TRY(hipMemcpy2DAsync(t_out, sizeof(double), c->tape.p + slot, (size_t)rows * c->N * sizeof(double), sizeof(double),
                                 (size_t)m, hipMemcpyDeviceToHost, c->stream));
    if (dt_dst)
        HIP_TRY(hipMemcpy2DAsync(dt_dst, sizeof(double), c->tape.p + (size_t)(supp ? 1 : 0) * c->N + slot,
                                 (size_t)rows * c->N * sizeof(double), sizeof(double), (size_t)m, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (!supp && t_out) {
        double t = c->tp.front();
        for (int k = 0; k < m; k++) { t_out[k] = t; t += dt_dst[k]; }
    }
    return CUDE_OK;
}

int32_t cude_loss_grad_partial(cude_ctx* c, double* partial, double* g_cond) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if (!partial) return fail(CUDE_ERR_ARG, "null output");
    if ((rc = run_ensemble(c, true, nullptr, /*local_only=*/true))) return rc;
    HIP_TRY(fetch(c, g_cond, c->g_cond.p, c->N));
    HIP_TRY(fetch(c, partial, c->g_nn.p, c->P + 2));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CUDE_OK;
}

int32_t cude_partial_buffer(cude_ctx* c, double** device_ptr, int32_t* count) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if (!device_ptr || !count) return fail(CUDE_ERR_ARG, "null output");
    if (!c->g_nn.p) return fail(CUDE_ERR_STATE, "context has no parameters yet");
    *device_ptr = c->g_nn.p;
    *count = c->P + 2;
    return CUDE_OK;
}

int32_t cude_loss_grad_partial_device(cude_ctx* c) {
    int32_t rc = bind(c);
    if (rc) return rc;
    if ((rc = run_ensemble(c, true, nullptr, /*local_only=*/true))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));     // the caller's collective runs on a stream this library does not know
    return CUDE_OK;
}

#ifdef CUDE_WAVE_TIMING
// development builds only: per-wave {start, end of forward sweep, end, hw id} of the last gradient launch
int32_t cude_debug_wave_timing(cude_ctx* c, long long* out, int64_t n_waves) {
    int32_t rc = bind(c);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, c->dbg.p, (size_t)std::min<int64_t>(n_waves, c->nblocks) * 4 * sizeof(long long),
                      hipMemcpyDeviceToHost));
    return CUDE_OK;
}
#endif

}  // extern "C"
