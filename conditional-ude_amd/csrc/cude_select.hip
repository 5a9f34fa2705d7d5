// libcude_hip.so -- launch selection: every rule that picks a launch shape from sizes and measurements (kept
// activations, one lane per subject / time-split / mixed and the chunk counts, issue priority, parameter sets per launch,
// speculation depths), each with the measurements that justify it.  The launches themselves are cude_launch.hip's.
//
// CUDE_SELECT_RULES_ONLY: the context-free integer rules alone, for a host test that includes this file
// (tests/cpp/select_rules.cpp).
#ifndef CUDE_SELECT_RULES_ONLY
#include "cude_ctx.h"
#else
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>
#endif

namespace cude {
namespace api {

// Parameter sets (grid points, candidates, output times ...) per launch: as many as there are, as the grid dimension
// that carries them holds and as fit the scratch budget at bytes_per_set each, at least one; an option that lowers the
// count (tests force several launches with it) applies last.
int64_t sets_per_launch(int64_t n, int64_t grid_cap, double budget_bytes, double bytes_per_set, int option_cap) {
    int64_t sets = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n, grid_cap), (int64_t)(budget_bytes / bytes_per_set)));
    if (option_cap > 0) sets = std::min<int64_t>(sets, option_cap);
    return sets;
}

namespace {
// the divisor d >= 2 of S nearest to `target` (the smaller of two equally near), 0 if S < 2
int nearest_divisor(int S, double target) {
    int best = 0;
    for (int d = 2; d <= S; d++)
        if (S % d == 0 && (best == 0 || std::fabs(d - target) < std::fabs(best - target))) best = d;
    return best;
}

// issue rate of a SIMD that holds w waves, relative to a lone wave's (profiles/r02/ubench_fma_latency.txt)
double shared_simd_rate(double w) { return w <= 1.0 ? 1.0 : (w <= 2.0 ? 1.33 : (w <= 3.0 ? 1.36 : 1.38)); }

// first step of each of L chunks of S steps, and S
std::vector<int32_t> chunk_starts(int S, int L) {
    std::vector<int32_t> cs(L + 1);
    for (int k = 0; k <= L; k++) cs[k] = (int32_t)((int64_t)k * S / L);
    return cs;
}
}  // namespace

#ifndef CUDE_SELECT_RULES_ONLY
// SUPP gradient launches keep the network activations of the forward sweep (instead of recomputing them in the
// reverse sweep) when that buffer is small: the launch is then latency-bound and 2/3 of the reverse sweep's
// instructions are worth 8*(D*W+1) bytes per evaluation; at 1e5 subjects the 2.3 GB each way would cost more than the
// recomputation.  Option "supp_store" = 0 / 1 overrides the size rule (tests, A/B runs).
size_t supp_act_doubles(const cude_ctx* c) {
    return (size_t)(6 * c->cfg.n_steps + 1) * (size_t)(c->net.depth * c->net.width + 1) * (size_t)c->N;
}
bool supp_keep_activations(const cude_ctx* c, int64_t n_sets) {
    if (c->net.general() || c->net.generic()) return false;      // (other activation functions / shapes: no kept activations)
    if (c->opt.supp_store == 0 || c->opt.supp_store == 1) return c->opt.supp_store == 1;
    return (double)n_sets * (double)supp_act_doubles(c) * 8.0 <= 256e6;
}

// c-peptide gradient launches (one lane per subject, single parameter set): option "cpep_keep" = 2 keeps the upper layers'
// activations of the forward sweep in HBM for the reverse sweep (CpepArgs::act; measured slower at the benchmark sizes,
// see cpep_kernel -- off unless asked for)
#ifndef CUDE_CPEP_KEEP_DEFAULT
#define CUDE_CPEP_KEEP_DEFAULT 0
#endif
size_t cpep_act_doubles(const cude_ctx* c) {
    const int nk = cude::cpep_keep_values(c->net);
    if (nk == 0 || c->cfg.n_steps == 0) return 0;
    const size_t nblocks = (size_t)((c->N + cude::kBlock - 1) / cude::kBlock);
    return (size_t)(5 * c->cfg.n_steps + 1) * (size_t)nk * nblocks * cude::kBlock;
}
// "cpep_keep" = 0 (recompute everything) | 1 (keep the output unit's logistic derivative) | 2 (keep the upper layers)
int cpep_keep_mode(const cude_ctx* c) {
    const int m = c->opt.cpep_keep ? c->opt.cpep_keep : CUDE_CPEP_KEEP_DEFAULT;
    return (m == 1 || m == 2) && cpep_act_doubles(c) > 0 ? m : 0;
}
bool cpep_keep_activations(const cude_ctx* c) { return cpep_keep_mode(c) != 0; }

// option "supp_ckpt" = "steps": gradient launches of the suppression model keep only the step states (744 B per subject at
// S = 30) and re-run the stages in the reverse sweep, instead of keeping every stage input (4.3 KB per subject)
bool supp_steps_only(const cude_ctx* c) { return c->opt.supp_ckpt_steps != 0; }

// chunks of a forward-only time-split launch: the forward-only split where there is one, otherwise the gradient's
int forward_chunks(const cude_ctx* c) { return c->chunks_f > 1 ? c->chunks_f : c->chunks; }

// Relative cost of one gradient launch when `waves` workgroups of `evals` network evaluations each run on `slots`
// resident-wave slots: full rounds cost one wave length each; a last partial round that leaves at least half of the
// SIMDs with a single wave runs at single-wave speed (measured on MI355X: a wave alone on its SIMD takes 0.69 of the
// time it takes next to a second one; profiles/r02/sweep_chunks.txt).
double launch_cost(double waves, double slots, double evals) {
    const double x = waves / slots;
    const double full = std::floor(x + 1e-9), frac = x - full;
    const double rounds = full + (frac < 1e-9 ? 0.0 : (frac <= 0.5 ? 0.69 : 1.0));
    return rounds * evals;
}

// Chunking of the step range for the time-split gradient path (1 <-> the one-lane-per-subject kernel; forced by
// CUDE_CPEP_PATH=1 / =2:L or an unsupported shape).  Precomputes the kinetics-only chunk transfer matrices.
//
// Choice of L (divisors of S): the launch that minimises launch_cost().  One lane per subject gives nblocks waves of
// 5S+1 evaluations; L chunks give nblocks*L waves of 5S/L+3 (two extra forward and one extra reverse evaluation per
// chunk).  Splitting pays when the one-shot grid would end in a mostly idle round -- 1e5 subjects = 1563 waves on
// 2048 slots took as long as 125 000 -- or leave the chip empty (57 subjects = one wave).  Measured (round 2, 2x6x6x1,
// S = 30): 1e5 subjects 0.644 -> 0.571 ms (L = 5), 8e4 0.637 -> 0.477 (L = 3), 2e5 1.222 -> 1.135 (L = 3), 125 000
// stays at L = 1 (0.654 vs 0.683 for L = 2).
int32_t setup_chunks(cude_ctx* c) {
    c->chunks = 1;
    c->chunks_f = 0;
    c->blk0 = 0;
    c->slots_one = c->half_slots = 0;
    int n_cu = 256;
    (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->cfg.device);
    c->n_cu = n_cu;
    c->half_slots = (int64_t)n_cu * 4;
    if (adaptive(c)) return CUDE_OK;
    c->slots_one = (int64_t)n_cu * std::max(1, cude::cpep_grad_waves_per_cu(c->net, c->cfg.n_state, c->T));
    c->half_slots = (int64_t)n_cu * 4;
    const int forced = c->opt.cpep_path;        // option "cpep_path": 0 = the cost model below decides
    if (forced == 1) return CUDE_OK;
    if (!cude::cpep2_shape_supported(c->net, c->cfg.n_state)) return CUDE_OK;
    const int S = c->cfg.n_steps;
    const int occ_rev = std::max(1, cude::cpep2_rev_waves_per_cu(c->net));
    const int occ_one = std::max(1, cude::cpep_grad_waves_per_cu(c->net, c->cfg.n_state, c->T));
    int L = 1;
    double best = launch_cost((double)c->nblocks, (double)n_cu * occ_one, 5.0 * S + 1.0);
    for (int d = 2; d <= S; d++) {
        if (S % d) continue;
        // (x 1.10: time-split launches of a whole population measure 8-10 % above this model, the one-lane launch on it --
        // 300 000 subjects: L = 3 modelled 9 % faster than one lane per subject, measured 7 % slower)
        const double cost = 1.10 * launch_cost((double)c->nblocks * d, (double)n_cu * occ_rev, 5.0 * S / d + 3.0);
        if (cost < best * (1.0 - 1e-3)) { best = cost; L = d; }
    }
    // Small populations (at most two workgroups per compute unit before splitting): the slot model above takes every
    // resident wave for full throughput, but a SIMD gives 1, 1.33, 1.36, 1.38 ... of a lone wave's rate to 1, 2, 3, 4+
    // waves (profiles/r02/ubench_fma_latency.txt) -- it chose 15 chunks for 1e4 and 2e4 subjects where 6 are 5 % and 11 %
    // faster, and 30 for 4 000 where 15 are 8 % faster (profiles/r05/sweep_chunks_small.txt).  Model fitted to that sweep:
    // a wave of 5S/L + 3 evaluations at 1.36 us each, slowed by the waves it shares its SIMD with, + 0.25 us of scan per chunk.
    if (c->nblocks <= 2 * (int64_t)n_cu) {
        const double simds = (double)n_cu * 4.0;
        int Ls = 0;
        double best_s = 0.0;
        for (int d = 2; d <= S; d++) {
            if (S % d) continue;
            const double w = std::ceil((double)c->nblocks * d / simds);
            const double cost = 1.36 * (5.0 * S / d + 3.0) * w / shared_simd_rate(w) + 0.25 * d;
            if (Ls == 0 || cost < best_s) { best_s = cost; Ls = d; }
        }
        if (Ls >= 2) L = Ls;
    }
    // Mixed launch (more than one machine-fill of subjects): whole rounds of the one-lane kernel, the remainder --
    // which would otherwise be a second, mostly idle round -- time-split on its own.  Cost = the two parts one after
    // the other (they do overlap at the seam; not counted).
    int64_t blk0 = 0;
    const int64_t slots_one = (int64_t)n_cu * occ_one;
    // Only between one and two machine-fills: with two or more whole rounds the one-lane launch's own tail is amortised
    // and the mixed launch measured slower (300 000 subjects 1.461 against 1.366 ms, 1e6 4.415 against 4.183 ms).
    if (c->nblocks > slots_one && c->nblocks < 2 * slots_one && c->opt.mixed) {
        const int64_t bulk = (c->nblocks / slots_one) * slots_one, rem = c->nblocks - bulk;
        if (rem > 0) {
            const double cost_bulk = launch_cost((double)bulk, (double)slots_one, 5.0 * S + 1.0);
            // chunks of ~6 steps for the remainder (measured best at 140 000 ... 200 000 subjects: L = 5 or 6 of S = 30)
            const int Lm = nearest_divisor(S, S / 6.0);
            if (Lm > 0) {
                const double cost = cost_bulk + launch_cost((double)rem * Lm, (double)n_cu * occ_rev, 5.0 * S / Lm + 3.0);
                if (cost < best * (1.0 - 3e-2)) { L = Lm; blk0 = bulk; best = cost; }
            }
        }
    }
    // Mixed launch below one machine-fill (between one and two waves per SIMD, register-limited one-lane kernel): one
    // long wave on every SIMD and the remainder as short waves in the second slot, side by side.  Measured on the
    // headline instance (profiles/r02/mixed_launch.txt): 1e5 subjects 0.549 -> 0.485 ms, 8e4 0.448 -> 0.402 ms, no gain
    // at 125 000 (0.610 vs 0.580) or at <= 65 536.  Model: the longer of the lone long wave (0.69 of its co-resident
    // time) and the whole work at two waves per SIMD, + 6 %; chunks of ~6 steps, ~3 for a small remainder.
    const int64_t half = (int64_t)n_cu * 4;
    if (blk0 == 0 && occ_one == 8 && c->nblocks > half && c->nblocks < slots_one && c->opt.mixed) {
        const int64_t rem = c->nblocks - half;
        const double target = S / (rem >= 300 ? 6.0 : 3.0);
        const int Lm = nearest_divisor(S, target);
        if (Lm > 0) {
            const double e1 = 5.0 * S + 1.0;
            const double cost = std::max(0.69 * e1, 1.06 * ((double)half * e1 + (double)rem * (5.0 * S + 3.0 * Lm)) / (double)slots_one);
            if (cost <= best) { L = Lm; blk0 = half; best = cost; }
        }
    }
    // Kernels that could hold three waves per SIMD (the reference's 2-4-4-1 / 2-state instance): a third resident wave
    // adds no throughput to the one-lane launch (0.45 ms with one or two waves per SIMD, 0.83 ms with three), which the
    // slot-count model above does not know.  Measured rule (profiles/r02/mixed_launch.txt, second table): from ~1.2
    // waves per SIMD up to two, one long wave per SIMD + the rest in chunks of ~3 steps (1e5 subjects 0.387 -> 0.369 ms);
    // between two and three, two long waves per SIMD + the rest in chunks of ~6 steps (150 000: 0.549 -> 0.494 ms,
    // 196 608: 0.834 -> 0.629 ms).
    if (blk0 == 0 && occ_one >= 12 && c->opt.mixed) {
        int64_t bulk = 0;
        double target = 0.0;
        if (c->nblocks >= half + half / 6 && c->nblocks <= half + 3 * half / 4) { bulk = half; target = S / 3.0; }
        else if (c->nblocks > half + 3 * half / 4 && c->nblocks <= 2 * half) L = 1;   // two waves per SIMD, taking turns at
                                                                                     // the issue priority: 0.428 ms up to 131 072
        else if (c->nblocks > 2 * half && c->nblocks <= 3 * half) { bulk = 2 * half; target = S / 6.0; }
        if (bulk > 0) {
            const int Lm = nearest_divisor(S, target);
            if (Lm > 0) { L = Lm; blk0 = bulk; }
        }
    }
    if (c->opt.debug_selector)
        fprintf(stderr, "[cude] chunk selector: nblocks=%lld CUs=%d waves/CU one-lane=%d reverse=%d -> L=%d, one-lane blocks %lld\n",
                (long long)c->nblocks, n_cu, occ_one, occ_rev, L, (long long)blk0);
    if (forced == 2) { L = c->opt.path_chunks; blk0 = 0; }
    if (forced == 3) {                                        // "3:<one-lane blocks>:<L>" (tests)
        blk0 = std::min<int64_t>(std::max<int64_t>(c->opt.path_blk0, 0), c->nblocks - 1);
        L = c->opt.path_chunks;
    }
    if (L > S) L = S;
    if (L < 2) return CUDE_OK;
    const std::vector<int32_t> cs = chunk_starts(S, L);
    const int64_t N = c->N;
    const int T = c->T;
    HIP_TRY(c->chunk_start.resize(L + 1));
    HIP_TRY(c->hom_M.resize((size_t)L * 4 * N));
    HIP_TRY(c->hom_obs.resize((size_t)T * 2 * N));
    HIP_TRY(c->fsum.resize((size_t)L * (3 + T) * N));
    HIP_TRY(c->res.resize((size_t)5 * S * N));   // adjoint weights wts[5S][N]
    HIP_TRY(c->g_cond_part.resize((size_t)L * N));
    HIP_TRY(c->partials2.resize((size_t)L * c->nblocks * c->P));
    HIP_TRY(push(c, c->chunk_start.p, cs.data(), cs.size()));
    c->chunks = L;
    c->blk0 = blk0;
    if (blk0 > 0 && !c->stream2 && !c->opt.mixed_one_stream) {
        HIP_TRY(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
    }
    cude::CpepArgs a = cpep_args(c);
    cude::Cpep2Args a2 = chunk_args(c, a);
    HIP_TRY(cude::cpep2_prepare());
    HIP_TRY(cude::launch_cpep2_homog(a2, c->stream));
    HIP_TRY(c->adj_map.resize((size_t)cude::adj_map_rows(T) * N));          // the scan's adjoint recursion as a linear map
    HIP_TRY(cude::launch_cpep2_adjmap(a2, c->adj_map.p, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));   // cs (host vector) dies here
    // ---- the forward-only split.  Model (fitted to profiles/r03/forward_chunks.txt): a SIMD that holds w waves of e
    // evaluations each needs e * w / thr(w) evaluation times (thr = 1, 1.33, 1.36, 1.38 ... for 1, 2, 3, 4+ waves: the
    // issue rates of profiles/r02/ubench_fma_latency.txt), e = 5S/L + 2, and the scan adds ~0.6 evaluation times per chunk.
    c->chunks_f = 0;
    if (c->opt.fwd_split && forced != 2 && forced != 3) {
        const double simds = (double)n_cu * 4.0;
        int Lf = 0;
        double best_f = 0.0;
        for (int d = 2; d <= S; d++) {
            if (S % d) continue;
            const double w = std::ceil((double)c->nblocks * d / simds);
            // (0.6 per chunk dates from the one-wave scan; the eight-wave scan stitches a chunk in ~0.1 us and plain forward
            //  calls of <= 2 000 subjects would gain ~1 us from 30 chunks instead of 15 -- but the speculative Metropolis
            //  rounds launch 3 or 7 parameter sets on this split, and with 30 chunks their waves no longer have a SIMD each:
            //  1 250 subjects x 100 steps 1.25 -> 1.34 ms.  Kept.)
            const double cost = (5.0 * S / d + 2.0) * w / shared_simd_rate(w) + 0.6 * d;
            if (Lf == 0 || cost < best_f) { best_f = cost; Lf = d; }
        }
        if (Lf >= 2 && Lf != L) {
            const std::vector<int32_t> csf = chunk_starts(S, Lf);
            HIP_TRY(c->chunk_start_f.resize(Lf + 1));
            HIP_TRY(c->hom_M_f.resize((size_t)Lf * 4 * N));
            HIP_TRY(c->hom_obs_f.resize((size_t)T * 2 * N));
            HIP_TRY(c->fsum_f.resize((size_t)Lf * (3 + T) * N));
            HIP_TRY(push(c, c->chunk_start_f.p, csf.data(), csf.size()));
            c->chunks_f = Lf;
            cude::Cpep2Args af = chunk_args(c, a, /*all_blocks=*/true, /*forward_only=*/true);
            HIP_TRY(cude::launch_cpep2_homog(af, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        if (c->opt.debug_selector)
            fprintf(stderr, "[cude] forward-only split: L_f=%d (gradient L=%d)\n", Lf, L);
    }
    return CUDE_OK;
}

// Alternating issue priority in the one-lane gradient kernel (CpepArgs::prio_shift): for a launch of `blocks` workgroups
// that is a single round with two waves on (some of) the SIMDs.  (Ablation builds: CUDE_PRIO_SHIFT=k overrides, 0 = never.)
int prio_shift_for(const cude_ctx* c, int64_t blocks) {
    if (c->opt.prio_shift >= 0) return c->opt.prio_shift;
    // two waves on (some of) the SIMDs and no third: also the kernels that could hold three (2-4-4-1 / 2 states at
    // 120 000 ... 131 072 subjects: 0.451 -> 0.426 ms); not the one-wave kernels (2-7-7-1: +2 %)
    return (c->slots_one >= 2 * c->half_slots && blocks > c->half_slots && blocks <= 2 * c->half_slots) ? 5 : 0;
}

// HOW the launches picked above take their turns (CpepArgs::prio_clock; option "prio_clock", ablation builds:
// CUDE_PRIO_CLOCK): 0 = every 2^prio_shift evaluations of each wave's own progress, k > 0 = every 2^k cycles of the shader
// clock the co-resident waves share.  Fixed-step c-peptide gradient kernel only: the adaptive kernels keep the
// progress-keyed form, their work per wave being data-dependent (run_ensemble never hands them a clock bit).
// Bit 17 = turns of 2^17 cycles, ~55 us, ~32 evaluations of the headline kernel: 125 000 subjects, 2-6-6-1 / 3 states,
// kernel ms by k: 14 0.508, 15 0.498, 16 0.495, 17 0.495, 18 0.494, 19 0.495, 20 and up slower than no turns at all (a turn outlasts the sweep),
// against 0.521 for the progress-keyed turns at their best common setting and 0.538 without (profiles/prio_clock.txt).
constexpr int kPrioClockBit = 17;
int prio_clock_for(const cude_ctx* c) {
    const int k = c->opt.prio_clock >= 0 ? c->opt.prio_clock : kPrioClockBit;
    return k < 62 ? k : 62;
}

// Bytes of scratch one multi-set launch may use (partial rows, stage inputs, tapes): sets per launch = this / the
// scratch of one set.  More sets per launch fill the chip better (25 sets of 1e5 subjects: 39 000 waves in one grid
// instead of 25 grids that each end in a part-filled round), and the per-set results do not depend on it.
double sets_scratch_budget(cude_ctx* c) {
    if (c->scratch_budget > 0.0) return c->scratch_budget;
    size_t free_b = 0, total_b = 0;
    c->scratch_budget = 512e6;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b >= ((size_t)64 << 30))
        c->scratch_budget = std::min(16e9, std::max(512e6, 0.25 * (double)free_b));
    else
        (void)hipGetLastError();
    return c->scratch_budget;
}

// Steps per speculative round of cude_mh_chain (0 = one step per launch pair, the plain fused path).  Option "mh_spec":
// 0 off, 2 ... 4 forced; -1 (default) by size: a round of depth d evaluates 2^d - 1 candidates per subject in one launch,
// which is nearly free while the candidates' forward chunks run side by side on otherwise idle SIMDs and costs their
// full multiple once the chip is filled.  Rule = waves of the round's forward launch (candidates x workgroups x chunks of
// the forward split): depth 3 while they fit two waves per SIMD (the resident-weights variant of the forward kernel),
// depth 2 up to ~3 per SIMD.  profiles/r05/estep_speculative.txt (one MI355X, 2-4-4-1, 100 steps, us per step plain ->
// speculative): 625 subjects 23.8 -> 12.2 (depth 3), 1 250: 23.9 -> 13.7 (2; 14.5 with 3), 1 600: 23.7 -> 16.0 (2; 14.6 with 3),
// 2 500: 23.6 -> 16.5 (2), 5 000: 25.7 -> 23.5 (2), 1e4: 30.9 -> 29.6 (2), 12 000 and above: slower, off.  With the
// eight-wave scan (which helps the plain step more) 1e4 is a draw (30.2 -> 29.6 in that tool, 30.1 -> 31.2 in bench.py's
// 1e4 x 100): off from ~8 000 subjects.
int mh_spec_depth(const cude_ctx* c, int n_mc) {
    int d = c->opt.mh_spec;
    if (d < 0) {
        const int64_t waves1 = c->nblocks * forward_chunks(c);
        d = 7 * waves1 <= 2048 ? 3 : (3 * waves1 <= 2400 ? 2 : 0);
    }
    d = std::min(d, cude::kMhSpecMaxDepth);
    if (d > n_mc) d = n_mc;
    return d >= 2 ? d : 0;
}

// The same speculation for the contexts whose forward solve is ONE launch over lanes = subjects (the adaptive solve -- the
// API mirrors' default --, the one-lane fixed-step kernel): a Metropolis step there is a wave's whole solve (84 us for
// 57 ... 1 000 subjects in the adaptive mode) on a chip that a small population leaves empty, so the 2^d - 1 candidate
// states run side by side as parameter sets of the launch (grid rows) and mh_spec_kernel resolves the d decisions.
// Depth while the candidates' workgroups still have a SIMD each (profiles/r05/estep_speculative.txt, adaptive mode, 100
// steps, ms per E-step plain -> depth 2 / 3 / 4: 57 subjects 10.4 -> 5.6 / 4.0 / 3.1, 1 000: 12.1 -> 6.3 / 4.5 / 3.5,
// 4 000: 12.4 -> - / 6.0 / 4.7, 1e4: 12.6 -> 8.7 / 8.3 / -).
int mh_spec_depth_one_launch(const cude_ctx* c, int n_mc) {
    int d = c->opt.mh_spec;
    if (d < 0) d = 15 * c->nblocks <= 1024 ? 4 : (7 * c->nblocks <= 1100 ? 3 : (3 * c->nblocks <= 1024 ? 2 : 0));
    d = std::min(d, cude::kMhSpecMaxDepth);
    if (d > n_mc) d = n_mc;
    return d >= 2 ? d : 0;
}

// gamma < 1, the proposal and both possible next states in one launch: d such steps per launch by speculation
// (MhSpecArgs::blend: a node of the candidate heap is its state AND its proposal, 2 (2^d - 1) parameter sets) while the
// sets' waves still have a SIMD each
// (profiles/r05/estep_speculative.txt, gamma = 0.25, 100 steps, ms per E-step two launches per step -> one -> depth
//  2 / 3: adaptive 57 subjects 20.3 -> 11.0 -> 5.6 / 4.0, 4 000: 24.0 -> 12.8 -> 8.7 / 6.0, 1e4: 24.3 -> 17.3 -> 8.7 /
//  11.5; fixed 30 steps (time-split) 57: 4.10 -> 2.39 -> 1.27 / 1.01, 1 000: 4.06 -> 2.39 -> 1.51 / 1.57, 4 000:
//  4.28 -> 3.68 -> 3.02 / 3.61, 1e4: 5.94 -> 6.17 -> 5.10 / 6.62)
int mh_spec_depth_blend(const cude_ctx* c, int n_mc, bool split) {
    int d = c->opt.mh_spec;
    if (d < 0) {
        const int64_t waves1 = c->nblocks * (split ? forward_chunks(c) : 1);
        if (split) d = 14 * waves1 <= 2048 ? 3 : (6 * waves1 <= 6000 ? 2 : 0);
        else d = 14 * waves1 <= 1024 ? 3 : (6 * waves1 <= 1024 ? 2 : 0);
    }
    d = std::min(std::min(d, (int)cude::kMhSpecMaxDepthBlend), n_mc);
    return d >= 2 ? d : 0;
}

// Probes per forward launch of cude_fit_conditional (option "fit_spec"; 0 = one probe per launch): every such launch is one
// wave's whole solve per 64 subjects, and a small population leaves the chip empty -- a golden-section step has two
// outcomes, so the probes of the next d steps are a heap of 2^d - 1 brackets evaluated together, 2 (2^d - 1) sets, while
// their waves still find room beside each other (fsplit: the time-split forward kernels, forward_chunks waves per workgroup)
int fit_spec_depth(const cude_ctx* c, bool fsplit) {
    int d = c->opt.fit_spec;
    if (d < 0) {
        const int64_t waves1 = c->nblocks * (fsplit ? forward_chunks(c) : 1);
        const int64_t room = fsplit ? 4096 : 1024;
        d = 30 * waves1 <= room ? 4 : (14 * waves1 <= room ? 3 : (6 * waves1 <= room ? 2 : 1));
    }
    if (c->net.generic()) d = 0;
    return std::min(d, (int)cude::kFitSpecMaxDepth);
}
#endif  // CUDE_SELECT_RULES_ONLY

}  // namespace api
}  // namespace cude
