// Internal header of libcude_hip.so's host side: the context, its helpers and what the translation units share.
//   cude_context.hip   contexts, populations, parameters, solver tables, run-time options
//   cude_select.hip    the measured rules that pick a launch shape (one-lane / time-split / mixed, sets per launch, depths)
//   cude_launch.hip    the launches themselves (ensemble, parameter sets, tangent, dense output) and the entry points that are one
//   cude_batch.hip     the entry points that batch such launches (simulate, bands, profiles, fits, scores, screening)
//   cude_replicates.hip  the entry points that simulate replicates of the data (bootstrap, npde, vpc, their draws)
//   cude_mh.hip        the Metropolis driver (cude_mh_estep, cude_mh_chain)
//   cude_optimise.hip  Adam (single steps and captured runs), L-BFGS on host vectors
//   cude_train.hip     restarts trained side by side with their optimiser state on the device (cude_train_restarts)
//   cude_lm.hip        Levenberg-Marquardt on the information matrices (cude_lm_candidates, cude_train_lm) and its kernels
//   cude_comm.hip      multi-GPU: RCCL (dlopen) and the peer-write exchange over IPC-mapped mailboxes
#pragma once
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/cude.h"
#include "cude_kernels.h"
#include "cude_optim.h"
#include "cude_passes.h"

namespace cude {
namespace api {

// thread-local text of the last error (cude_last_error); returns `code`
int32_t fail(int32_t code, const std::string& msg);

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return ::cude::api::fail(CUDE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));  \
    } while (0)

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    hipError_t resize(size_t count) {
        if (count == n) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; n = 0; }
        if (count == 0) return hipSuccess;
        hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
    // grow-only variant for scratch that is reused across calls
    hipError_t reserve(size_t count) { return count <= n ? hipSuccess : resize(count); }
    ~DevBuf() { if (p) (void)hipFree(p); }
};

// Run-time options of a context.  cude_set_option(ctx, name, value) sets one; at cude_create every option whose
// environment variable is set (table in cude_context.hip) takes that value.  The second group exists for A/B
// measurements only: the shipping library reads their environment variables in -DCUDE_ABLATION builds alone.
struct Options {
    int cpep_path = 0;          // "cpep_path" / CUDE_CPEP_PATH: "" = the cost model chooses; "1" = one lane per subject;
    int path_chunks = 0;        //   "2:L" = time-split into L chunks; "3:B:L" = mixed, blocks [0, B) one-lane, rest in L chunks
    int64_t path_blk0 = 0;
    int cpep_keep = 0;          // "cpep_keep" / CUDE_CPEP_KEEP: 0 recompute, 1 keep the logistic derivative, 2 keep the upper layers
    int supp_store = -1;        // "supp_store" / CUDE_SUPP_STORE: -1 = size rule, 0 / 1 = never / always keep activations
    int supp_ckpt_steps = 0;    // "supp_ckpt" / CUDE_SUPP_CKPT: "steps" = keep step states only, re-run the stages in reverse
    int tape_steps = 0;         // "tape_steps" / CUDE_TAPE_STEPS: capacity of the adaptive gradient tape (0 = sized to ~4 GB)
    int exp_table = 1;          // "exp_table" / CUDE_NO_EXPTAB: layer-1 exponent recurrence along glucose pieces
    int ms_split = 1;           // "ms_split" / CUDE_NO_MS_SPLIT: restarts of a small population on the time-split kernels
    int train_host = 0;         // "train_host" / CUDE_TRAIN_HOST: 1 = cude_train_restarts keeps the L-BFGS vectors on the host
                                //   (what a sharded population always does), 2 = the Adam stage on the host as well
    int mh_spec = -1;           // "mh_spec" / CUDE_MH_SPEC: speculative Metropolis steps per launch chain (cude_mh_estep, gamma == 1,
                                //   time-split forward path): 0 = off, 2 ... 4 = that many, -1 = by population size (mh_spec_depth)
    int fit_spec = -1;          // "fit_spec" / CUDE_FIT_SPEC: cude_fit_conditional with several probes per forward launch (the grid scan
                                //   as parameter sets, the next d golden-section steps as a heap of brackets): 0 = one probe per launch,
                                //   1 ... 4 = that depth, -1 = by population size
    int adaptive_team = 1;      // "adaptive_team" / CUDE_NO_ADAPTIVE_TEAM: adaptive launches of small c-peptide populations put a
                                //   step's five network evaluations on five waves (cude_adaptive_team.hip)
    int auto_regroup = 1;       // "auto_regroup" / CUDE_NO_AUTO_REGROUP: adaptive launches re-ordered by accepted-step count
    int poll_pinned = 1;        // "poll_pinned" / CUDE_NO_POLL_PINNED: watch page-locked result slots instead of the stream wait
    int force_fallback = 0;     // "force_fallback" / CUDE_FORCE_FALLBACK (tests): cude_set_network takes the fallback kernel also
                                //   for shapes a tuned kernel is compiled for
    int debug_selector = 0;     // "debug_selector" / CUDE_DEBUG_SELECTOR: print the launch-path decision
    int xchg_allow_plain = 0;   // "xchg_allow_plain" / CUDE_ALLOW_PLAIN_MAILBOX: ordinary device memory as a mailbox although
                                //   peers sit on other devices (the owner's polls may then be served from its L2)
    int xchg_fail_kinds = 0;    // "xchg_fail_kinds" / CUDE_XCHG_FAIL_KINDS (tests): bit k set = this rank's cude_xchg_attach
                                //   reports a failure when its mailbox is of the k-th memory kind (0 uncached, 1 fine-grained, 2 plain)
    int dense_chunk = 0;        // "dense_chunk" / CUDE_DENSE_CHUNK: cude_simulate's output times per launch (0 = ~1 GB of scratch)
    int dense_layout = 0;       // "dense_layout" / CUDE_DENSE_LAYOUT: suppression dense output written straight into the caller's
                                //   [3 x T x N] (0, measured faster: cude_simulate) or lane-contiguous [T][3][N] + a transpose (1)
    int refine_fused = 1;       // "refine_fused" / CUDE_REFINE_FUSED: cude_refine_conditional in fixed-step mode as ONE launch (1) or as one
                                //   tangent launch + one update launch per evaluation (0: the form the adaptive mode always runs)
    int profile_chunk = 0;      // "profile_chunk" / CUDE_PROFILE_CHUNK: grid points per launch of cude_profile_conditional / cude_profile_intervals
                                //   (0 = as many as ~512 MB of scratch allow; tests force several launches with it)
    int predictive_subjects = 0; // "predictive_subjects" / CUDE_PREDICTIVE_SUBJECTS: subjects per solve launch of cude_predictive_bands,
                                //   rounded up to whole workgroups of 64 (0 = as many as ~1 GB of sample trajectories allow)
    int predictive_times = 0;   // "predictive_times" / CUDE_PREDICTIVE_TIMES: its output times per launch (0 = all of them unless 64
                                //   subjects alone exceed that budget); tests force several launches in either dimension with them
    int bootstrap_chunk = 0;    // "bootstrap_chunk" / CUDE_BOOTSTRAP_CHUNK: replicates per launch of cude_bootstrap_conditional (0 = as many
                                //   as ~256 MB of replicate observations allow)
    int bootstrap_subjects = 0; // "bootstrap_subjects" / CUDE_BOOTSTRAP_SUBJECTS: its subjects per pass, rounded up to whole workgroups of
                                //   64 (0 = as many as ~1 GB of replicate results allow); tests force either split with them
    int npde_subjects = 0;      // "npde_subjects" / CUDE_NPDE_SUBJECTS: subjects per pass of cude_npde, rounded up to whole workgroups of 64
                                //   (0 = as many as ~1 GB of trajectories and simulated observations allow); tests force the split with it
    int vpc_sims = 0;           // "vpc_sims" / CUDE_VPC_SIMS: simulations per pass of cude_vpc (0 = as many as ~1 GB of trajectories and
                                //   simulated observations allow); tests force the split with it
    int vpc_select = 0;         // "vpc_select" / CUDE_VPC_SELECT (tests): 1 = every column of cude_vpc's reduction over subjects goes
                                //   through the radix select, whatever its length
    // ("hidden_activation" = tanh | relu | sigmoid, "output_activation" = softplus | identity: kept in cude_ctx::net)
    // ---- ablation
    int mixed = 1;              // CUDE_NO_MIXED
    int mixed_one_stream = 0;   // CUDE_MIXED_ONE_STREAM
    int fwd_split = 1;          // CUDE_NO_FWD_SPLIT
    int fused_final = 1;        // CUDE_NO_FUSED_FINAL
    int fused_tail = 1;         // CUDE_NO_FUSED_TAIL: tail of a time-split gradient evaluation in one launch (round 5)
    int scan_bulk = 1;          // CUDE_NO_SCAN_BULK: small scan launches fetch every row through LDS up front (round 5)
    int scan_map = 1;           // CUDE_NO_SCAN_MAP: the scan's adjoint recursion as a per-subject linear map (round 5)
    int mh_fuse = 1;            // CUDE_NO_MH_FUSE
    int mh_pair = 1;            // CUDE_NO_MH_PAIR: gamma < 1 -- the proposal and both possible next states in one launch (round 5)
    int graph = 1;              // CUDE_NO_GRAPH
    int graph_unroll = 8;       // CUDE_GRAPH_UNROLL
    int prio_shift = -1;        // CUDE_PRIO_SHIFT (-1 = the rule in prio_shift_for)
    int prio_clock = -1;        // CUDE_PRIO_CLOCK: the launches that alternate do so by their own progress (0) or by the shader clock,
                                //   period 2^k cycles (k > 0); -1 = the rule in prio_clock_for
    int lean_clamp = -1;        // CUDE_LEAN_CLAMP: -1 = the fixed-step gradient kernel's waves drop the clamps their parameter set
                                //   proves dead (CpepArgs::lean_clamp, the kernel's own test); 0 = always the clamped sweeps
};

// Peer-write exchange (cude_comm.hip): this rank's mailbox, every rank's mailbox as mapped here, per-column sequence
// counters and the status word on the device.  ready: attached, self-tested and switched on.
struct Exchange {
    bool ready = false;         // the reductions of run_ensemble go through it
    bool attached = false;
    int kind = 0;               // how the mailbox was allocated: 3 uncached, 1 fine-grained, 0 plain device memory
    int kind_index = 0;         // position of `kind` in the order of preference (0 uncached, 1 fine-grained, 2 plain)
    uint64_t* box = nullptr;    // own mailbox [2][n_ranks][cols][2] words
    size_t box_words = 0;
    int cols = 0;
    uint64_t* peers[CUDE_XCHG_MAX_RANKS] = {};
    bool opened[CUDE_XCHG_MAX_RANKS] = {};      // mapped through hipIpcOpenMemHandle (to be closed)
    uint32_t* seq = nullptr;    // [cols]
    int32_t* status = nullptr;  // set by a wait that ran out of time: the device's address of status_host
    int32_t* status_host = nullptr;     // page-locked, coherent: the host reads it after any synchronisation, no copy
    double timeout_s = 20.0;
};

}  // namespace api
}  // namespace cude

// bit pattern the host puts into every slot of cude_ctx::pinned_pairs before a launch it is going to watch: a quiet NaN
// with a payload no arithmetic produces
constexpr uint64_t kPairSentinel = 0x7ff8dead5eed0001ull;

struct cude_ctx {
    cude_config cfg;
    cude::api::Options opt;
    cude::NetShape net;
    int P = 0;
    hipStream_t stream = nullptr;
    int64_t N = 0;          // local subjects
    double n_global = 0;    // subjects over all ranks
    int T = 0;
    std::vector<double> tp;
    bool have_pop = false, have_nn = false, have_cond = false;
    // population (CPEP)
    cude::api::DevBuf<double> k0, k1, k2, c0, dG, obs, age;
    // population (SUPP)
    cude::api::DevBuf<double> data, ckpt;
    double scale[3] = {1, 1, 1};
    // tables
    cude::api::DevBuf<int32_t> seg, obs_step, stepk;
    cude::api::DevBuf<double> phi, obs_w, stepd, tp_dev;
    cude::api::DevBuf<double> supp_rho, supp_obs_rho;   // SUPP, fixed step: state 1 per evaluation / observation relative to u1(t_0)
    double abstol = 1e-6, reltol = 1e-3;   // adaptive mode (n_steps == 0): OrdinaryDiffEq's defaults
    // parameters / gradients / optimiser
    cude::api::DevBuf<double> nn, cond, g_nn, g_cond, sse, auc, partials, traj;
    cude::api::DevBuf<double> sens, sens_info, sens_score;     // cude_sensitivity: [n_state x T x N], [N], [N] (first call)
    cude::api::DevBuf<double> sens2, sens_curv;                // cude_curvature: [n_state x T x N], [N] (first call)
    cude::api::DevBuf<double> refine_buf;                      // cude_refine_conditional: 13 rows of N (first call; kept, so that
    cude::api::DevBuf<int32_t> refine_ibuf;                    // ... repeated fits -- SAEM's MAP step -- do not allocate): 2 rows
    // chunked gradient path (cude_cpep2.hip)
    int chunks = 1;
    int n_cu = 256;         // compute units of the device (setup_chunks)
    int64_t blk0 = 0;       // > 0: mixed gradient launch -- blocks [0, blk0) on the one-lane kernel, the rest time-split
    int64_t slots_one = 0, half_slots = 0;          // resident-wave slots of the one-lane gradient kernel; one per SIMD
    hipStream_t stream2 = nullptr;                  // mixed launch: the time-split remainder runs beside the whole rounds
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    cude::api::DevBuf<double> param_mask;                      // frozen shared parameters (cude_set_param_mask); empty = none
    std::vector<double> mask_host;
    cude::api::DevBuf<int32_t> chunk_start;
    cude::api::DevBuf<double> hom_M, hom_obs, fsum, res, g_cond_part, partials2;
    // forward-only launches of the time-split path have their own split (chunks_f, 0 = the gradient's): the scan's cost
    // grows with the chunk count and there is no reverse kernel to feed, so fewer, longer chunks win there
    int chunks_f = 0;
    cude::api::DevBuf<int32_t> chunk_start_f;
    cude::api::DevBuf<double> hom_M_f, hom_obs_f, fsum_f;
    cude::api::DevBuf<double> m_nn, v_nn, m_cond, v_cond;
    int64_t nblocks = 0;
    double lr = 1e-3, b1 = 0.9, b2 = 0.999, eps = 1e-8;
    int64_t adam_t = 0;
    bool adam_ready = false;
    cude::api::DevBuf<double> adam_state, adam_trace;   // device-resident step state and per-iteration loss trace
    int64_t trace_cap = 0;
    // cude_adam_run: captured optimiser iterations -- graph [u] holds 2^u of them back to back (kernels of one graph
    // follow each other without a gap; between two graph launches the GPU idles ~8 us, tools/step_gaps.py); a run of
    // n iterations is its binary decomposition, largest graphs first (8 at most: CUDE_GRAPH_UNROLL)
    static constexpr int kGraphKinds = 4;
    hipGraph_t graph[kGraphKinds] = {nullptr, nullptr, nullptr, nullptr};
    hipGraphExec_t graph_exec[kGraphKinds] = {nullptr, nullptr, nullptr, nullptr};
    bool capturing = false;
    int32_t timing_period = 1;      // kernel timing: events around every timing_period-th ensemble launch
    int64_t timing_count = 0;
    // Adam state advance (running powers, step counter, loss trace): folded into the kernel that finishes an iteration's
    // [sum loss, n_failed] when the iteration is run by cude_adam_step / cude_adam_run (fold_advance), otherwise -- and
    // with a communicator but no L2 term, where the pair is final only after the all-reduce -- its own launch
    bool fold_advance = false, advance_done = false;
    int64_t last_failed = 0;
    // comm: an RCCL communicator and / or the peer-write exchange (cude_comm.hip); either makes the context "distributed"
    void* comm = nullptr;
    int n_ranks = 1, rank = 0;
    cude::api::Exchange xchg;
    int32_t xchg_timeouts = 0;      // device-side waits of the exchange that gave up so far (cude_xchg_info)
    int xchg_next_kind = 0;         // first memory kind the next cude_xchg_export tries (advanced by a failed attach / a detach)
    // timing of the dominant kernel
    bool timing = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    uint64_t rng_seed = 0x243F6A8885A308D3ull;      // device-side draws of the Metropolis steps (cude_set_rng)
    int64_t rng_offset = 0, rng_step = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    size_t ev_used = 0;
    double host_red[3];
    double* pinned = nullptr;       // page-locked staging of the small result vectors ([g_nn; loss sum; n_failed])
    // set by a caller right before run_ensemble when finish_loss(loss, nullptr) follows at once and is the call's ONLY
    // pending output: then the result slots in page-locked memory may be watched instead of waiting for the stream (a
    // launch whose result nobody fetches must not write there: a later call's watch would take it for its own)
    bool allow_watch = false;
    bool poll_pairs = false;
    bool poll_ok = true;            // cleared by the first watch that timed out: host memory is not coherent here
    bool tail_in_pinned = false;    // the tail reduction of the last launch also wrote [sum loss, n_failed] to pinned[P..P+1]
    double* pinned_pairs = nullptr; // page-locked [nblocks][2]: per-workgroup (sum SSE, failures) of a forward-only launch,
    int64_t pinned_pairs_n = 0;     // written by the scan kernel itself and added up by the host (finish_loss)
    bool loss_in_pinned = false;    // the last forward launch left its result there
    // scratch of cude_multistart_loss_grad (kept between calls: it is called once per optimiser iteration)
    cude::api::DevBuf<double> ms_nn, ms_cond, ms_part, ms_out, ms_gcond, ms_ckpt, ms_act;
    cude::api::DevBuf<double> ms_fsum, ms_wts, ms_gcp, ms_p2;   // time-split path with parameter sets (small populations)
    cude::api::DevBuf<double> act;     // SUPP: kept network activations of the gradient launch (small populations only)
    cude::api::DevBuf<double> tape, ms_tape;   // adaptive mode: accepted steps of the forward sweep, walked back by the adjoint
    cude::api::DevBuf<double> adj_map;             // time-split path: Cpep2Args::adj_map of the population
    cude::api::DevBuf<double> gen_acc, ms_gacc;    // general network (cude_generic.hip): [P][N] gradient accumulators per set
    cude::api::DevBuf<int32_t> tape_n;
    cude::api::DevBuf<int32_t> perm;                           // adaptive kernels: subject of every launch position (cude_adaptive_regroup)
    std::vector<int32_t> slot_of;                   // its inverse on the host (empty = identity)
    int64_t run_iters = 0;                          // iterations cude_adam_run has made on this population
    int64_t regroup_done_at = -1;                   // ... and the count at which it last re-ordered the launch by itself
    int tape_cap = 0;
    bool have_tape = false;         // the tape of the last gradient evaluation is readable (it is in the current launch order)
    bool have_counts = false;       // tape_n holds every subject's accepted-step count of some adaptive evaluation
    int64_t evals_since_regroup = 0;
    cude::api::DevBuf<double> red_tmp; // staging of small host vectors reduced through the communicator
    cude::api::DevBuf<double> ms_f;    // per-set loss values of a multi-set evaluation
    cude::api::DevBuf<double> sc_rows, sc_sets, sc_state, sc_part;     // cude_subject_scores: rows table, per-set rows, fold state,
    cude::api::DevBuf<int32_t> sc_int;                                 // ... cross-product partials; kept between calls
    cude::api::DevBuf<double> ni_state, ni_stage;                      // cude_network_information: fold state and matrices, the
                                                                       // staging of a chunk's rows as [N][outputs][P]
    cude::api::DevBuf<double> lm_buf, lm_part;                         // cude_lm_candidates / cude_train_lm: the damped steps'
    cude::api::DevBuf<int32_t> lm_int;                                 // ... tables and trial sets, the trial launch's partials
    double scratch_budget = 0.0;       // bytes of scratch one multi-set launch may use (sets_scratch_budget)
    // cude_train_restarts (cude_train.hip): the restarts' optimiser state, resident between iterations
    cude::api::DevBuf<double> tr_m_nn, tr_v_nn, tr_m_cond, tr_v_cond, tr_trace;     // Adam moments [K][P] / [K][N], loss trace
    cude::api::DevBuf<int32_t> tr_alive, tr_act;
    cude::api::DevBuf<double> tr_x, tr_g, tr_d, tr_s, tr_y, tr_trial, tr_gtrial;    // L-BFGS vectors [R][N + P], history [R][m][N + P]
    cude::api::DevBuf<unsigned char> tr_state;
    void* tr_pinned = nullptr;         // page-locked copy of the L-BFGS states / alive flags the host reads once per round
    size_t tr_pinned_bytes = 0;
#ifdef CUDE_WAVE_TIMING
    cude::api::DevBuf<long long> dbg;
#endif
};

namespace cude {
namespace api {

// both c-peptide models share the population layout, solver tables and the ensemble kernel
inline bool is_cpep(const cude_ctx* c) { return c->cfg.model == CUDE_MODEL_CPEP || c->cfg.model == CUDE_MODEL_CPEP_SYM; }

inline bool adaptive(const cude_ctx* c) { return c->cfg.n_steps == 0; }
inline double step_size(const cude_ctx* c) { return adaptive(c) ? 0.0 : (c->tp.back() - c->tp.front()) / c->cfg.n_steps; }
inline bool distributed(const cude_ctx* c) { return c->comm != nullptr || c->xchg.ready; }

inline int32_t bind(cude_ctx* c) {
    if (!c) return fail(CUDE_ERR_ARG, "null context");
    HIP_TRY(hipSetDevice(c->cfg.device));
    return CUDE_OK;
}

// ---- cude_context.hip
void interp_weights(double theta, double* w7);      // h-free dense-output weights b_i(theta) of Tsit5
// suppression model, fixed step: state 1 at outputs (step[k], w[k][0..6]) relative to u1(t_0) (SuppArgs::obs_rho)
void supp_output_rho(int S, double h, const std::vector<int32_t>& step, const std::vector<double>& w, std::vector<double>& obs_rho);
int32_t apply_option(cude_ctx* c, const char* name, const char* value);
// plain one-dimensional copies on the context's stream, asynchronous, the byte count taken from the element type
template <class T>
hipError_t push(const cude_ctx* c, T* dst, const T* src, size_t n) {       // host -> device
    return hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyHostToDevice, c->stream);
}
template <class T>
hipError_t fetch(const cude_ctx* c, T* dst, const T* src, size_t n) {      // device -> host; null dst: an output nobody asked for
    return dst ? hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, c->stream) : hipSuccess;
}

// A buffer cut into consecutive arrays.  The layout is written once, as a function of a Carve: run on a null base it
// measures (take returns null, `used` is the size), run on the buffer it hands out the pointers -- carve() does both.
template <class T>
struct Carve {
    T* base;
    size_t used = 0;
    T* take(size_t n) {
        T* const p = base ? base + used : nullptr;
        used += n;
        return p;
    }
};
template <class T, class Layout>
hipError_t carve(DevBuf<T>& buf, Layout layout) {
    Carve<T> size{nullptr};
    layout(size);
    const hipError_t e = buf.reserve(size.used);
    if (e != hipSuccess) return e;
    Carve<T> v{buf.p};
    layout(v);
    return hipSuccess;
}

// adaptive launches leave every subject's accepted-step count behind (of set 0 where there are several); tape_valid: the
// launch was the gradient evaluation whose tape cude_adaptive_steps pairs those counts with
inline void note_adaptive_launch(cude_ctx* c, bool tape_valid) {
    if (!adaptive(c)) return;
    c->have_counts = true;
    c->have_tape = tape_valid;
}

// ---- cude_select.hip
size_t supp_act_doubles(const cude_ctx* c);
bool supp_keep_activations(const cude_ctx* c, int64_t n_sets);
size_t cpep_act_doubles(const cude_ctx* c);
int cpep_keep_mode(const cude_ctx* c);
bool cpep_keep_activations(const cude_ctx* c);
bool supp_steps_only(const cude_ctx* c);
int32_t setup_chunks(cude_ctx* c);
int forward_chunks(const cude_ctx* c);
int prio_shift_for(const cude_ctx* c, int64_t blocks);
int prio_clock_for(const cude_ctx* c);
double sets_scratch_budget(cude_ctx* c);
constexpr int64_t kNoGridCap = std::numeric_limits<int64_t>::max();
int64_t sets_per_launch(int64_t n, int64_t grid_cap, double budget_bytes, double bytes_per_set, int option_cap = 0);
int mh_spec_depth(const cude_ctx* c, int n_mc);
int mh_spec_depth_one_launch(const cude_ctx* c, int n_mc);
int mh_spec_depth_blend(const cude_ctx* c, int n_mc, bool split);
int fit_spec_depth(const cude_ctx* c, bool fsplit);
// ---- cude_launch.hip
cude::CpepArgs cpep_args(const cude_ctx* c);
cude::SuppArgs supp_args(const cude_ctx* c);
cude::Cpep2Args chunk_args(cude_ctx* c, const cude::CpepArgs& base, bool all_blocks = false, bool forward_only = false);
int generic_tape_rows(const cude_ctx* c);
int64_t tape_doubles_per_set(const cude_ctx* c);
int32_t ensure_tape(cude_ctx* c);
int32_t timed_pair(cude_ctx* c, hipEvent_t* e0, hipEvent_t* e1);
int32_t run_ensemble(cude_ctx* c, bool grad, double* traj_dev, bool local_only = false, const double* cond_ov = nullptr,
                     double* sse_ov = nullptr);
int32_t finish_loss(cude_ctx* c, double* loss, double* g_nn_host);
int32_t adaptive_regroup(cude_ctx* c, int32_t* spread_before, int32_t* spread_after);
int32_t maybe_regroup(cude_ctx* c);
struct SetsRows {
    double* rows;            // [n_sets][P][N]: row of subject i in set k (CpepArgs::lane_rows)
    double* sse;             // [n_sets][N]
    int32_t unit_seed = 0;   // 1 + l0 > 0: set k's reverse sweep is seeded with 1.0 at live output l0 + k (CpepArgs::unit_seed)
};
int32_t eval_sets_device(cude_ctx* c, int64_t n_sets, const double* nn, int64_t stride_nn, const double* cond,
                         int64_t stride_cond, double* g_cond, double* out, const SetsRows* rows = nullptr);
// obs_ov: observations to read instead of the population's, in its layout (obs [T][N] / data [3][T][N])
hipError_t launch_tangent(cude_ctx* c, const double* cond, double* sse, const cude::SensOut& out, bool keep_tape,
                          const double* obs_ov = nullptr);
// ... one order-2 solve (cude_curv.hip): `out.sens` is not written, `out2` holds the second-order outputs
hipError_t launch_tangent2(cude_ctx* c, const double* cond, double* sse, const cude::SensOut& out, const cude::CurvOut& out2,
                           bool keep_tape);
// A forward solve of n_sets parameter sets in one launch (set k: nn + k * stride_nn, cond + k * N; the set index is a grid
// dimension): what the entry points that batch solves differ in.  The rest of the launch is forward_sets's.
struct SetsForward {
    const double* cond = nullptr;       // [n_sets][N]
    const double* nn = nullptr;         // stride_nn = 0: one network for every set
    int64_t stride_nn = 0;
    int n_sets = 0;
    double* sse = nullptr;              // [n_sets][N] per-subject SSE, or null
    double* partials = nullptr;         // [n_sets][nblocks][P + 2] of a launch that is not split: [sum SSE, failures] in
                                        // the last two columns (reserve_sets_forward)
    bool split = false;                 // the time-split forward kernels (c-peptide models, fixed step, chunks > 1)
    const cude::MhSpecArgs* resolve_in_scan = nullptr;      // split only: the scan launch resolves this speculative round
};
int32_t reserve_sets_forward(cude_ctx* c, int64_t max_sets, bool split, DevBuf<double>& own_part);
int32_t forward_sets(cude_ctx* c, const SetsForward& s);
// Dense output (cude_simulate, cude_predictive_bands).  The tables of ALL output times of a call, on the device: in
// fixed-step mode the step every output falls into, its seven interpolation weights and, for the suppression model, state 1
// there; in adaptive mode the times themselves (the kernel interpolates at them).  An entry depends on its own time
// alone, so launches over a stretch of the times point into the tables.
struct OutputTables {
    DevBuf<int32_t> d_step;
    DevBuf<double> d_w, d_rho, d_times;
    int32_t upload(cude_ctx* c, int64_t n_times, const double* times);      // (queued; the host copies live as long as this)
  private:
    std::vector<int32_t> step;
    std::vector<double> w, rho;
};
// One outputs-only launch: output times [k0, k0 + kn) of the tables, the states to `traj`.
struct DenseLaunch {
    const double* cond = nullptr;       // [N], or [n_sets][N]
    int32_t n_sets = 0;                 // 0: one set (the launch's second grid dimension otherwise; one network for all)
    int64_t set_stride = 0;             // set k writes traj + k * set_stride
    int64_t k0 = 0, kn = 0;
    double* traj = nullptr;             // c-peptide models: [n_state x kn x N] per set
    int64_t traj_ss = 0, traj_st = 0, traj_sn = 0;      // suppression model: state s, output o, subject i at s ss + o st + i sn
    double* partials = nullptr;
    bool keep_perm = true;              // adaptive mode: false = the caller's order, not the re-grouped launch order
    int64_t blk_first = 0, blk_count = 0;       // workgroups [blk_first, blk_first + blk_count) of the population (0: all)
};
int32_t launch_dense(cude_ctx* c, const OutputTables& tables, const DenseLaunch& d);
// Simulate and observe (cude_npde, cude_vpc; cude_replicates.hip): what a call's passes share.  The caller's arguments, and
// the device side that prepare() allocates for passes of at most sets_max simulations of sub_max subjects in `blocks`
// workgroups: the sets [sets][N], sigma [N] (uploaded), the trajectories [sets][subjects][T][NS] at the data's own times
// (whose tables it uploads), the simulated observations y [sets][T - 1][subjects] and their flags used [sets][subjects].
struct SimObserve {
    const double* cond_sets = nullptr;  // host [n_sims][N]; null: drawn on the device around (prior_mean, prior_sd)
    double prior_mean = 0.0, prior_sd = 0.0;
    const double* noise = nullptr;      // host [n_sims][T - 1][N]; null: drawn on the device
    int64_t first_rep = 0;
    int32_t state = 0;
    DevBuf<double> d_cond, d_sigma, d_slab, d_y, d_part;
    DevBuf<uint8_t> d_used;
    OutputTables tables;
    int32_t prepare(cude_ctx* c, const double* sigma, int64_t sets_max, int64_t sub_max, int64_t blocks);
};
// One pass, queued: simulations [k0, k0 + kn) of subjects [s0, s0 + sn), s0 a multiple of the workgroup's 64.  With
// `place` the sets are uploaded or drawn first (all N subjects of them); then the 0xff fill of adaptive mode, the solve, the
// caller's noise into y, the observations.  The pass's results start at the heads of slab, y and used.
int32_t simulate_observe_pass(cude_ctx* c, const SimObserve& v, int64_t s0, int64_t sn, int64_t k0, int64_t kn, bool place);
// ---- cude_batch.hip
// The device half of cude_network_information, shared with the Levenberg-Marquardt entry points (cude_lm.hip).
struct InfoRequest {
    const double* cond = nullptr;       // host [N]; null: the context's conditionals
    double pw = 0.0;
    const double* cov = nullptr;        // host [P][P], with want_q
    bool profiled = false;
    double* jac_out = nullptr;          // host [N][n_out][P], written chunk by chunk
    bool want_a = false, want_schur = false, want_q = false;
};
struct InfoTables {
    cude::InfoArgs ia;                  // b [P][N], d [N], jc, qf [N][n_out], status [N] on the device
    double *gn = nullptr, *schur = nullptr, *coup = nullptr;    // [P][P], [P][P], staging of the coupling table as [N][P]
    int32_t* nfail = nullptr;           // device: failed subjects
    int32_t failed = 0;                 // its host copy: final after the next synchronisation of the stream
};
int32_t info_pass(cude_ctx* c, const InfoRequest& rq, InfoTables& tb);
// The per-subject fits in their stepped form and their search state, shared with the bootstrap (cude_replicates.hip)
hipError_t refine_stepped(cude_ctx* c, const cude::RefineCfg& k, const cude::RefineArrays& r, double* sse_t, double* score_t,
                          double* info_t, const double* obs_ov);
int32_t refine_state(cude_ctx* c, cude::RefineArrays& r, double** sse_t, double** score_t, double** info_t);
// ---- cude_optimise.hip
void drop_graph(cude_ctx* c);
int32_t ensure_trace(cude_ctx* c, int64_t n);
cude::TailAdvance tail_advance(cude_ctx* c);
int32_t enqueue_adam(cude_ctx* c);
// ---- cude_comm.hip
// sum (op 0) / max (op 1) of a device vector over the ranks, in place, on the context's stream (identity on one rank)
int32_t allreduce_dev(cude_ctx* c, double* buf, size_t count, int op = 0);
int32_t comm_reduce_host(cude_ctx* c, double* values, int32_t count, int op);
int32_t lbfgs_comm_reduce(double* values, int32_t count, int32_t op, void* user);
cude::XchgArgs xchg_args(const cude_ctx* c);
int32_t xchg_check(cude_ctx* c);           // after a synchronisation: CUDE_ERR_COMM if a device-side wait ran out of time
void xchg_release(cude_ctx* c);
void comm_release(cude_ctx* c);

}  // namespace api
}  // namespace cude
