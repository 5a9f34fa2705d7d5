// Kernel argument blocks and host-side launch entry points (implemented in the .hip files).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cude_xchg.h"

namespace cude {

constexpr int kBlock = 64;     // one wave per workgroup: no cross-wave barrier on the path
constexpr int kMaxObs = 32;

// activation functions a network can be built with (`chain(widths, activations; output_activation)`,
// src/neural-network.jl:42-58); tanh / softplus are what every script of the reference uses
constexpr int kActHiddenTanh = 0, kActHiddenRelu = 1, kActHiddenSigmoid = 2, kActHiddenIdentity = 3;
constexpr int kActOutSoftplus = 0, kActOutIdentity = 1;

// The general network (cude_generic.hip): per-layer widths and activation functions, evaluated by the fallback kernel
// when no tuned kernel is compiled for the shape.  Activation codes = CUDE_ACT_* of include/cude.h.
constexpr int kGenMaxLayers = 9;                 // hidden layers + the output layer
constexpr int kGenActTanh = 0, kGenActRelu = 1, kGenActSigmoid = 2, kGenActSoftplus = 3, kGenActIdentity = 4;
constexpr size_t kGenMaxLds = 160 * 1024;        // a workgroup's LDS on gfx950
struct GenNet {
    int32_t n_layers = 0;                        // 0 = not a general network
    int32_t nin = 0;
    int32_t width[kGenMaxLayers] = {};           // units of layer l (the last layer: 1)
    int32_t act[kGenMaxLayers] = {};
    __host__ __device__ int n_params() const {
        int p = 0, fan = nin;
        for (int l = 0; l < n_layers; l++) { p += width[l] * fan + width[l]; fan = width[l]; }
        return p;
    }
    __host__ __device__ int n_units() const {
        int u = 0;
        for (int l = 0; l < n_layers; l++) u += width[l];
        return u;
    }
    __host__ __device__ int max_width() const {
        int m = 0;
        for (int l = 0; l < n_layers; l++) m = width[l] > m ? width[l] : m;
        return m;
    }
};
size_t gen_lds_bytes(const GenNet& net);         // LDS of one workgroup of the fallback kernel

struct NetShape {
    int nin, width, depth;
    int hact = kActHiddenTanh, oact = kActOutSoftplus;
    GenNet gen;                                  // gen.n_layers > 0: the fallback kernel evaluates THIS network
    bool generic() const { return gen.n_layers > 0; }
    bool general() const { return hact != kActHiddenTanh || oact != kActOutSoftplus; }
    bool symbolic() const { return width == 0 && !generic(); }   // analytic production p0*dG/(dG+k): P = 1
    int n_params() const {
        if (generic()) return gen.n_params();
        if (symbolic()) return 1;
        int p = 0, fan = nin;
        for (int l = 0; l < depth; l++) { p += width * fan + width; fan = width; }
        return p + fan + 1;
    }
};

// c-peptide cUDE (linear kinetics + state-independent NN forcing)
struct CpepArgs {
    int64_t N;
    const double* k0; const double* k1; const double* k2; const double* c0;   // [N]
    const double* dG;        // [T][N]  glucose(t_j) - glucose(t_0)
    const double* obs;       // [T][N]
    const double* age;       // [N] (covariate model) or nullptr
    const double* cond;      // [N]
    const double* nn;        // [P]
    const int32_t* seg;      // [S*5]  glucose segment of each distinct stage time
    const double* phi;       // [S*5]  fraction inside the segment
    const int32_t* obs_step; // [T]
    const double* obs_w;     // [T][7] h-free dense-output weights b_i(theta)
    // layer-1 exponent table of the network kernels: per step {kind in the forward sweep, kind in the reverse
    // sweep, glucose piece of the step} with kind 0 = the step straddles a knot (direct exponentials), 1 = first
    // step of a run inside one piece (build table + anchor), 2 = continues the run; and per step {fraction of
    // t_n and of t_{n+1} inside the piece, h / piece length}
    const int32_t* stepk;    // [S][3]
    const double* stepd;     // [S][3]
    int32_t T, S;
    double h, inv_n;
    double* sse;             // [N] or nullptr
    double* traj;            // [NS x T x N] column-major or nullptr
    double* auc;             // [N] or nullptr (NS == 3: cumulative secretion at t_end)
    double* g_cond;          // [n_sets][N] (grad)
    double* partials;        // [n_sets][nblocks][P+2]
    double* act;             // one-lane gradient kernel: [nblocks][5S+1][(D-1)W+1][64] kept activations of the forward
                             // sweep (tanh outputs of the hidden layers 2..D + the output unit's logistic derivative per
                             // evaluation), read back by the reverse sweep instead of re-evaluating those layers;
                             // nullptr = recompute.
    int32_t keep_mode;       // with act: 1 = only the logistic derivative is kept ([nblocks][5S+1][64]), 2 = all of the above
    // multi-start evaluation: n_sets parameter sets in the grid's y dimension, set k reads nn + k*set_stride_nn and
    // cond + k*set_stride_cond (and writes sse / g_cond + k*set_stride_cond); 0/0/0 for the single-set path
    int32_t n_sets;
    int64_t set_stride_nn, set_stride_cond;
    int32_t cond_raw;        // symbolic model only: 1 = k is the conditional itself, 0 = k = exp(conditional)
    // adaptive mode (S == 0, cude_adaptive.hip): glucose knot times, output times (T of them; obs[T][N] when the
    // outputs are the observations) and the solver tolerances
    const double* tp;        // [TG] knot times = the population's timepoints
    int32_t TG;
    const double* out_times; // [T]
    double t_begin, t_end;   // integration span = the population's time span
    double abstol, reltol;
    // mixed launch of a large population (single parameter set): the one-lane kernel takes blocks [0, blk_count)
    // (0 = all of them), the time-split kernels blocks [blk0, nblocks)
    int64_t blk0, blk_count;
    int32_t prio_shift;      // one-lane gradient kernel: co-resident waves alternate issue priority every 2^prio_shift
                             // evaluations (0 = off); set by the host for single-round launches with two waves per SIMD
    int32_t prio_clock;      // how the turns are timed where prio_shift > 0: 0 = by each wave's own progress (above; all the adaptive
                             // kernels know), k > 0 = by bit k of the shader clock, i.e. every 2^k cycles (fixed-step kernel only)
    double* tape;            // adaptive gradient: [n_sets][tape_cap][N] step sizes dt_n of the accepted steps (+ T saved outputs)
    int32_t tape_cap;
    int32_t unit_seed;       // kernels compiled with ROWS only (cude_network_information): 0 = the reverse sweep is seeded with
                             // the residuals, as ever; 1 + l0 > 0 = set k seeds LIVE output l0 + k with exactly 1.0 and every
                             // other output with exactly 0.0 (unit_seed_cpep / unit_seed_supp, cude_device.h), so that the
                             // lane's row is d yhat_io / d theta and its g_cond d yhat_io / d cond_i.  SSE and failures: as ever.
                             // HERE, in the four bytes of padding between tape_cap and tape_n, not at the end: the argument
                             // block keeps its size and every other field its offset, so every kernel that does not read the
                             // field is the machine code it was (appended, the block grows to 648 bytes and the compiler orders
                             // the scalar loads of 91 gradient kernels of cude_cpep.hip differently: profiles/jacobian.txt)
    int32_t* tape_n;         // [N] accepted steps per subject of parameter set 0 (forward and gradient launches), or nullptr
    int32_t team;            // adaptive mode, small launches: 0 = a step's five evaluations on five waves (cude_adaptive_team.hip)
                             // where that kernel applies, -1 = never (option "adaptive_team" = 0)
    int32_t lean_clamp;      // fixed-step gradient kernel of the lean shapes (Mlp::HAS_LEAN; cpep_kernel, cude_cpep.hip): non-zero =
                             // a wave whose own parameter set passes Mlp::lean_ok runs the sweeps without the clamps of the
                             // layers above the first and of the output unit (the same bits); 0 = every wave runs the clamped
                             // sweeps.  No value forces the clamp-free form past the kernel's test.  In the four bytes of padding
                             // behind `team`, for unit_seed's reason: every other field keeps its offset.
    double* gen_acc;         // fallback kernel (cude_generic.hip), gradient: [n_sets][P][N] per-lane accumulators; its tape
                             // (CpepArgs::tape) is [n_sets][steps][2 + n_state][N] with steps = S, or tape_cap when S == 0
    const int32_t* perm;     // adaptive kernels: lane `gid` works on subject perm[gid] (nullptr = identity).  Lanes of a wave
                             // run as long as the slowest of them: cude_adaptive_regroup orders the subjects by their
                             // accepted-step counts so that a wave's lanes finish together.  The tape is kept in LANE order.
    // dense output of several parameter sets (cude_predictive_bands): set k writes traj + k * traj_set_stride; forward
    // launches start at workgroup blk_first of the population and cover blk_count of them (0 / 0 / 0: as ever)
    int64_t traj_set_stride, blk_first;
#ifdef CUDE_WAVE_TIMING
    long long* dbg;          // development builds only: [nblocks][4] = {start, end of forward, end, hw id} per wave
#endif
    double* lane_rows;       // gradient launches of the one-lane kernels (cude_subject_scores): [n_sets][P][N], entry q of the
                             // network gradient of subject i in set k at ((k P + q) N + i) -- gen_acc's layout -- as the lane
                             // holds it right before the workgroup's reduction; at the SUBJECT's index, also under perm.
                             // nullptr = not wanted.  The fallback kernel keeps this table anyway: its gen_acc IS the table.
};

// SAEM E-step (Metropolis-Hastings)
// z == nullptr / MhArgs::u == nullptr: the draw comes from the counter-based generator (RngKey) instead of a host row
struct RngKey {
    uint64_t seed;             // Philox key
    int64_t subject_offset;    // global index of local subject 0 (draws do not depend on how subjects are sharded)
    int64_t step;              // index of the Metropolis step since cude_set_rng
};
struct MhArgs {
    int64_t N;
    double* p;                 // chain state (conditional parameters), updated in place
    const double* prop;        // proposals
    const double* u;           // uniform draws of this step
    const double* sse_new; double* sse_cur;
    int32_t carry_sse;         // gamma == 1: the accepted proposal IS the next state, so its SSE is carried over
    int64_t* accepted;         // per-subject acceptance counter
    double prior_mean, prior_sd, ll_const, inv_2s2, temperature, gamma;
    RngKey key;                // used when u == nullptr
};

// Speculative Metropolis (gamma == 1, carried SSE): the chain state after a step is one of two values and the draws are
// known in advance (counter-based on (seed, subject, step), or the caller's rows), so the 2^d - 1 proposals that d
// consecutive steps CAN make are evaluated in ONE ensemble launch (candidate = parameter set) and the accept / reject
// decisions resolved afterwards: the same chain bit for bit, one dependent launch chain per d steps instead of per step.
// Candidates form a binary heap: node v (1-based; level l = floor(log2 v)) proposes q(v) = s(v) + std * z_l from its
// state s(v); s(1) = the chain state, s(2v) = s(v) (rejected), s(2v + 1) = q(v) (accepted).  cand / sse_sets: [v - 1][N].
constexpr int kMhSpecMaxDepth = 4;
constexpr int kMhSpecMaxDepthBlend = 3;     // gamma < 1 (MhSpecArgs::blend): two parameter sets per node
struct MhSpecArgs {
    MhArgs mh;                 // p, sse_cur, accepted, the prior and likelihood constants; key.step is NOT used (steps below)
    int32_t depth_resolve;     // levels of `cand` / `sse_sets` to resolve into the chain now (0: none -- the first call)
    int32_t depth_next;        // levels of candidates to write for the next round (0: none -- the last call)
    int64_t step_resolve, step_next;   // Metropolis step index of level 0 of either (device draws: the counter's step)
    const double* sse_sets;    // SSE of the candidates being resolved
    double* cand;              // read (resolve), then overwritten with the next round's
    const double* z_rows;      // caller's normals of the NEXT round's steps, row l at z_rows + l * N; nullptr = device draws
    const double* u_rows;      // caller's uniforms of the steps being RESOLVED, likewise
    double proposal_std;
    double* samples;           // chain state after every resolved step, row l at samples + l * N; or nullptr
    int32_t blend;             // gamma < 1: every node carries its state AND its proposal (mh_spec_resolve_blend, cude_rng.h):
                               //   cand / sse_sets rows [v - 1] = state of node v, [nodes + v - 1] = its proposal; depth <= 3
};
hipError_t launch_mh_spec(const MhSpecArgs& a, hipStream_t s);

// chunked loss+gradient path (cude_cpep2.hip): the S steps of every subject are split into L chunks
struct Cpep2Args {
    CpepArgs base;
    int32_t L;
    const int32_t* chunk_start;  // [L+1] step boundaries
    double* hom_M;               // [L][4][N]   chunk transfer matrix d y_out / d y_in (static per population)
    double* hom_obs;             // [T][2][N]   d y1(tau) / d y_in(chunk of tau)            (static)
    double* fsum;                // [L][3+T][N] forced chunk response: v1, v2, quadrature, obs parts
    double* wts;                 // [5S][N]     adjoint weight of every network evaluation (gradient only)
    double* g_cond_part;         // [L][N]
    double* partials2;           // [L][nblocks][P]
    // fused Metropolis step (forward-only launches): the forward chunks evaluate at the PROPOSAL state + std * draw
    // instead of base.cond, and the scan accepts / rejects it right where the SSE is formed -- two launches per
    // Metropolis step instead of four (propose, forward, scan, accept)
    // forward-only calls on one parameter set and one rank: every scan workgroup also writes its (sum SSE, failures)
    // pair straight into page-locked host memory mapped into the device, final_host[2 * workgroup + {0, 1}], and the
    // host adds the pairs up in workgroup order behind the synchronisation it performs anyway: no reduction launch and
    // no copy kernel behind the scan (two dispatches per forward call instead of four).  nullptr = off.
    double* final_host;
    int32_t mh_fused;
    const double* mh_z;          // [N] normals of this step, or nullptr = device stream (mh.key)
    double mh_std;
    MhArgs mh;
    // speculative Metropolis round (MhSpecArgs): spec_slots = 2^d > 0 makes the scan launch hold ALL candidate sets of a
    // subject in one workgroup (lane = slot * (64 / spec_slots) + local subject; slot = candidate set, the last slot
    // idles) and resolve the round right behind the SSEs -- no reduction, no resolver launch
    int32_t spec_slots;
    MhSpecArgs spec;
    int32_t defer_chunk_sum;     // gradient launches: leave g_cond_part to the caller's launch_chunked_tail (no sum_chunks launch)
    // The scan's adjoint recursion as a per-subject LINEAR MAP (round 5): the stage-adjoint algebra of a step (J_f = A, fixed
    // h) maps (lam1, lam2, kap1, kap2) of step n + 1 and the residual seeds of step n to those of step n and to the step's
    // five network weights with coefficients that depend on the subject's kinetics alone.  Rows of N doubles, computed once
    // per population by running the algebra on unit inputs (cpep2_adjmap_kernel): [0, 16) Phi[out][in], [16, 36) W[weight][in],
    // [36 + 9 oi, 36 + 9 oi + 9) response of (lam1, lam2, kap1, kap2, w0 ... w4) to a unit seed of observation oi.
    // 36 multiply-adds of depth 4 per step instead of ~100 of depth ~25; nullptr = the stage-by-stage algebra.
    const double* adj_map;
    // > 0: a scan launch of at most this many workgroups requests every row it will read up front, through LDS
    // (cpep2_scan_bulk_kernel: one memory round trip instead of a dozen dependent ones); 0 = never
    int64_t scan_bulk_blocks;
};
constexpr int kAdjMapRows = 36;
inline int64_t adj_map_rows(int T) { return kAdjMapRows + 9 * (int64_t)T; }
hipError_t launch_cpep2_adjmap(const Cpep2Args& a, double* adj_map, hipStream_t s);
hipError_t cpep2_prepare();
bool cpep2_shape_supported(const NetShape& net, int n_state);
int cpep2_rev_waves_per_cu(const NetShape& net);
int cpep_grad_waves_per_cu(const NetShape& net, int n_state, int T);
int cpep_keep_values(const NetShape& net);
hipError_t launch_cpep2_homog(const Cpep2Args& a, hipStream_t s);
// forward (+ scan) only when !grad: per-subject SSE and the loss partials, no trajectory output
hipError_t launch_cpep2(const NetShape& net, int n_state, bool grad, const Cpep2Args& a, hipStream_t s);

// suppression cUDE (nonlinear: NN input is the state)
// rows of N doubles in one parameter set's gradient scratch
// (states 2 and 3 only: state 1 is parameter-independent and never stored, cude_supp.hip)
inline __host__ __device__ int64_t supp_ckpt_rows(int S, int T) { return (int64_t)(6 * S + 1) * 2 + 2 * (int64_t)T; }

struct SuppArgs {
    int64_t N;
    const double* data;      // [3][T][N]
    const double* cond;      // [N]
    const double* nn;        // [P]
    const int32_t* obs_step; // [T]
    const double* obs_w;     // [T][7]
    int32_t T, S;
    double h, inv_n;
    double iscale2[3];       // 1/scale_s^2
    double* ckpt;            // [n_sets][supp_ckpt_rows][N]: [6S+1][2] stage inputs of states 2, 3 (linearisation points of
                             // the reverse sweep), then [T][2] their residuals
    const double* rho;       // [6S+1] fixed-step mode: state 1 at evaluation e = u1(t_0) * rho[e] (Tsit5 on du1 = -0.4 u1:
                             // a constant of the step size alone), wave-uniform
    const double* obs_rho;   // [T] ... and at observation oi = u1(t_0) * obs_rho[oi] (its dense output)
    double* act;             // [n_sets][6S+1][D*W+1][N] kept network activations, or nullptr = recompute them
    int32_t ckpt_steps_only; // 1: ckpt holds only the step states [S+1][2][N]; the reverse sweep re-runs the stages
    double* sse;             // [N] or nullptr (already divided by scale^2)
    double* traj;            // [3 x T x N] column-major or nullptr
    double* g_cond;          // [n_sets][N]
    double* partials;        // [n_sets][nblocks][P+2]
    int32_t n_sets;          // multi-start evaluation, as CpepArgs
    int64_t set_stride_nn, set_stride_cond;
    const double* out_times; // adaptive mode (S == 0): [T] observation times
    double t_begin, t_end;
    double abstol, reltol;
    double* tape;            // adaptive gradient, as CpepArgs
    int32_t tape_cap;
    int32_t unit_seed;       // as CpepArgs (in the padding behind tape_cap, likewise)
    int32_t* tape_n;
    double* gen_acc;         // as CpepArgs
    const int32_t* perm;     // as CpepArgs
    // outputs-only launches (dense output, cude_simulate), selected by T_data > 0: T counts the output times (obs_step /
    // obs_w / obs_rho or out_times hold T entries), T_data is the time stride of `data`, whose first column is u0.  No
    // residual, no SSE, no partials: the states go to traj[s * traj_ss + oi * traj_st + i * traj_sn] (subject i).
    int32_t T_data;
    int64_t traj_ss, traj_st, traj_sn;
    // ... of several parameter sets (cude_predictive_bands): set k writes traj + k * traj_set_stride; the launch starts at
    // workgroup blk_first of the population and covers blk_count of them (0 = the rest); 0 / 0 / 0: as ever
    int64_t traj_set_stride, blk_first, blk_count;
    double* lane_rows;       // as CpepArgs
};
// workgroups of a one-lane launch: the whole population, or the stretch the argument block names
template <class A>
inline int64_t launch_blocks(const A& a) { return a.blk_count > 0 ? a.blk_count : (a.N + kBlock - 1) / kBlock; }

// Forward-mode (tangent-linear) solves, cude_sensitivity (cude_sens.hip): the population and solver fields of the model's
// own argument block, and the three per-subject outputs of the tangent (any of them nullptr = not wanted).  Blocks of their
// own, so that the argument blocks of every other kernel stay what they are.  One parameter set, one lane per subject.
struct SensOut {
    double* sens = nullptr;  // [n_state x T x N] column-major: d u_s(t_j) / d cond_i
    double* info = nullptr;  // [N] sum over the observed outputs of (w * d yhat / d cond)^2
    double* score = nullptr; // [N] sum of w^2 (yhat - y) d yhat / d cond
};
struct CpepSensArgs : CpepArgs {
    SensOut out;
};
struct SuppSensArgs : SuppArgs {
    SensOut out;
};
// hipErrorInvalidValue when no tuned kernel is compiled for the shape (the fallback kernel has no tangent)
hipError_t launch_cpep_sens(const NetShape& net, int n_state, const CpepSensArgs& a, hipStream_t s);
hipError_t launch_supp_sens(const NetShape& net, const SuppSensArgs& a, hipStream_t s);

// Order-2 forward-mode solves, cude_curvature (cude_curv.hip): cude_sensitivity's blocks plus the two second-order outputs
// (`out.sens` is not written by these launches).  One parameter set, one lane per subject.
struct CurvOut {
    double* sens2 = nullptr; // [n_state x T x N] column-major: d^2 u_s(t_j) / d cond_i^2
    double* curv = nullptr;  // [N] info + sum of w^2 (yhat - y) d^2 yhat / d cond^2 = (1/2) d^2 SSE_i / d cond_i^2
};
struct CpepCurvArgs : CpepSensArgs {
    CurvOut out2;
};
struct SuppCurvArgs : SuppSensArgs {
    CurvOut out2;
};
// hipErrorInvalidValue when no tuned kernel is compiled for the shape, as launch_*_sens
hipError_t launch_cpep_curv(const NetShape& net, int n_state, const CpepCurvArgs& a, hipStream_t s);
hipError_t launch_supp_curv(const NetShape& net, const SuppCurvArgs& a, hipStream_t s);

// the fallback kernel for networks no tuned kernel is compiled for (net.generic(); cude_generic.hip)
hipError_t launch_cpep_generic(const NetShape& net, int n_state, bool grad, const CpepArgs& a, hipStream_t s);
hipError_t launch_supp_generic(const NetShape& net, bool grad, const SuppArgs& a, hipStream_t s);
// returns hipSuccess, or hipErrorInvalidValue when the shape is not compiled in
hipError_t launch_cpep(const NetShape& net, int n_state, bool grad, const CpepArgs& a, hipStream_t s);
hipError_t launch_supp(const NetShape& net, bool grad, const SuppArgs& a, hipStream_t s);
// outputs-only launch of the fixed-step tuned kernels (SuppArgs::T_data > 0; cude_supp_dense.hip); launch_supp routes here
hipError_t launch_supp_dense(const NetShape& net, const SuppArgs& a, hipStream_t s);
// [T][3][N] (lane-contiguous dense output) -> [N][T][3] (the column-major [3 x T x N] of the caller)
hipError_t launch_supp_traj_transpose(int64_t N, int T, const double* src, double* dst, hipStream_t s);
bool cpep_shape_supported(const NetShape& net, int n_state);
bool supp_shape_supported(const NetShape& net);
int supp_grad_waves_per_cu(const NetShape& net);
// adaptive Tsit5 (grad: + the adjoint of the accepted step sequence, needs args.tape); launch_cpep / launch_supp
// route here when args.S == 0
hipError_t launch_cpep_adaptive(const NetShape& net, bool grad, const CpepArgs& a, hipStream_t s);
hipError_t launch_supp_adaptive(const NetShape& net, bool grad, const SuppArgs& a, hipStream_t s);
// rows of N doubles per accepted step on the adaptive gradient's tape.  Suppression model (3 states): (t_n, dt_n, y_n) and
// the inputs of stages 2..7 (states 2 and 3; state 1's follow from y_n in closed arithmetic) -- the linearisation points
// of the reverse sweep, which then needs no network evaluation of its own (the one-body kernel of cude_adaptive.hip
// re-runs the stages from y_n and leaves those rows unused).  C-peptide models (2 states, constant Jacobian): dt_n
// alone -- the reverse sweep needs the stage times only and steps back from the final time.
constexpr int kSuppTapeHead = 5;                   // t_n, dt_n, y_n[3]
constexpr int kSuppTapeRows = kSuppTapeHead + 6 * 2;
inline __host__ __device__ int adaptive_tape_rows(int n_state) { return n_state == 3 ? kSuppTapeRows : 1; }
// ... and of one parameter set's tape: the steps, then per observation the saved output (c-peptide: state 1) or the
// residual's derivative with respect to states 2 and 3 (suppression)
inline __host__ __device__ int64_t adaptive_tape_rows(int n_state, int cap, int T) {
    return (int64_t)cap * adaptive_tape_rows(n_state) + (n_state == 3 ? 2 : 1) * T;
}

// common kernels
// out[q] = sum_b partials[b][stride*b + q] (fixed order, deterministic) for q in [col0, col0+ncol); with n_sets > 1
// the same for every set k: partials + k*nblocks*stride -> out + k*stride
// Adam state advance + loss-trace entry, folded into the kernel that produces an iteration's final [sum loss, n_failed]
// (the reduction of the two tail columns, or the L2 term behind it) or run on its own before the update kernel.
struct TailAdvance {
    double* state = nullptr;   // {b1^t, b2^t, steps done, trace position}; nullptr: nothing to advance
    double b1 = 0.0, b2 = 0.0;
    double* trace = nullptr;   // [cap][2] = (sum loss, n_failed) per iteration
    int64_t cap = 0;
};
// adv (optional; the launch must cover the tail columns stride-2, stride-1 and not accumulate): the workgroup of the
// failure-count column also sums the loss column and advances the optimiser state with the pair
// xchg (optional; the launch's columns must be final, i.e. not be accumulated into by a later launch): every column's sum
// goes through the exchange and `out` receives the sum over all ranks; with adv the tail workgroup exchanges both tail
// columns itself (the loss column's workgroup leaves them to it)
hipError_t launch_reduce_cols(const double* partials, int64_t nblocks, int stride, int col0, int ncol, double* out,
                              hipStream_t s, int n_sets = 1, const double* mask = nullptr, int n_mask = 0,
                              int out_stride = 0 /* doubles between the sets' output rows; 0 = stride */,
                              bool accumulate = false /* add to out instead of overwriting it */,
                              const TailAdvance* adv = nullptr,
                              double* host_tail = nullptr /* page-locked [2]: the sums of the last two columns as well */,
                              const XchgArgs* xchg = nullptr);
// The whole tail of a time-split gradient evaluation as ONE launch (chunked_tail_kernel, cude_common.hip): the network
// gradient from the reverse chunks' rows, the loss / failure columns from the scan's rows (with the tail work of
// launch_reduce_cols), and the chunks' shares of d loss / d conditional added up (g_cond_part == nullptr: not that part).
struct ChunkedTailArgs {
    const double* partials2; int64_t rows2;    // [n_sets][rows2][P]
    const double* partials; int64_t rows;      // [n_sets][rows][P + 2]
    int P;
    double* out; int out_stride;               // [n_sets][out_stride >= P + 2]
    const double* mask; int n_mask;
    TailAdvance adv; double* host_tail; XchgArgs xchg;
    const double* g_cond_part; int L; int64_t N; double* g_cond; int64_t g_cond_set_stride;
};
hipError_t launch_chunked_tail(const ChunkedTailArgs& a, int n_sets, hipStream_t s);
// buf[0..count) <- sum (op 0) / max (op 1) over the ranks, in place, through the exchange (any count: columns in turn)
hipError_t launch_xchg_allreduce(const XchgArgs& x, double* buf, int64_t count, int op, hipStream_t s);
hipError_t launch_adam_advance(const TailAdvance& adv, const double* g_tail, hipStream_t s);
// out[2k], out[2k+1] = sum_b partials[k][b][col0], [col0+1]  for k < n_sets (multi-start screening)
hipError_t launch_reduce_sets(const double* partials, int n_sets, int64_t nblocks, int stride, int col0, double* out,
                              hipStream_t s);
// screening: per-set losses and the running top-k of `partialsortperm(losses, 1:n_keep)`
hipError_t launch_set_losses(int n_sets, const double* sums, const double* nn, int P, double lambda, double n_global,
                             double* loss, hipStream_t s);
struct TopkArgs {
    int n_keep, n_have, n_new;
    long long first;                 // global index of the chunk's first candidate
    const double* best_loss; const long long* best_idx;     // [n_have]
    const double* chunk_loss;                                // [n_new]
    double* work;                                            // [n_have + n_new]
    double* new_loss; long long* new_idx; int* sel_src;      // [n_keep]
};
hipError_t launch_topk_merge(const TopkArgs& a, int P, int64_t N, const double* old_nn, const double* old_cond,
                             const double* chunk_nn, const double* chunk_cond, double* new_nn, double* new_cond,
                             hipStream_t s);
// g_nn[q] += 2*lambda*nn[q];  out[P] += lambda*sum(nn^2)*n_global   (so that loss = out[P]/n_global)
hipError_t launch_l2_term(const double* nn, int P, double lambda, double n_global, double* out, hipStream_t s,
                          const double* mask = nullptr, const TailAdvance* adv = nullptr);
struct AdamArgs {
    int64_t N; int P;
    double* cond; double* m_cond; double* v_cond; const double* g_cond;
    double* nn; double* m_nn; double* v_nn; const double* g_nn;   // g_nn[P+1] = n_failed
    double lr, b1, b2, eps, c1, c2;   // c1 = 1-b1^t, c2 = 1-b2^t (filled on the device from `state`)
    double* state;                    // device: {b1^t, b2^t, steps done, trace position}, ALREADY advanced to this step
};
hipError_t launch_adam(const AdamArgs& a, hipStream_t s);

// ---- restarts trained side by side with their optimiser state on the device (cude_train.hip)
// Behind a multi-set gradient evaluation (eval_sets_device): per set k the L2 term in l2_term_kernel's arithmetic,
// the loss value, and -- for the Adam stage -- the set's liveness and its loss-trace entry.
struct FinishSetsArgs {
    int P;
    double* out;             // [K][P+2]: in [masked g_nn; sum SSE; failures]; g_nn gets its L2 term in place (g_dst == nullptr)
    const double* nn;        // set k's network parameters at nn + k * stride_nn
    int64_t stride_nn;
    double lambda, n_global;
    const double* mask;      // [P] or nullptr
    double* f;               // [K] loss values, +Inf for a set with a failed subject
    double* g_dst;           // optional: the finished network gradient goes to g_dst + k * g_stride instead
    int64_t g_stride;
    int32_t* alive;          // optional [K]: cleared for a set whose loss is not finite (the reference drops that restart)
    double* trace;           // optional [K][trace_len]: trace[k][trace_pos] = loss of a live set
    int64_t trace_len, trace_pos;
};
hipError_t launch_finish_sets(const FinishSetsArgs& a, int n_sets, hipStream_t s);
// Optimisers.Adam for K sets at once, in the arithmetic of cude::adam_update (cude_optim.h; no contraction): dead sets skipped
struct AdamSetsArgs {
    int64_t N; int P;
    double* cond; double* nn;                       // [K][N], [K][P]
    double* m_cond; double* v_cond; double* m_nn; double* v_nn;
    const double* g_cond;                           // [K][N]
    const double* out;                              // [K][P+2] (network gradients)
    const int32_t* alive;                           // [K]
    double lr, b1, b2, eps, c1, c2;                 // c = 1 - b^t of this step (host: std::pow)
};
hipError_t launch_adam_sets(const AdamSetsArgs& a, int n_sets, hipStream_t s);
// Optim's L-BFGS + BackTracking (cude_optim.h) with the vectors of R restarts on the device: one state per restart,
// one workgroup per restart and round.  Vector layout [conditional (N); network (P)].
constexpr int kLbfgsM = 10;
constexpr int kLbfgsFirst = 0, kLbfgsFinite = 1, kLbfgsArmijo = 2, kLbfgsDone = 3;
struct LbfgsState {
    int32_t phase, pseudo, it, calls, accepted, f_flat, converged, ls_it, n_eval, maxiters, line_search_failed, pad_;
    double f, f0, dphi0, a1, a2, phi1, g_tol;
    double rho[kLbfgsM];
};
struct LbfgsArgs {
    int64_t n;               // N + P
    LbfgsState* state;       // [R]
    const int32_t* act;      // [A]: restart of every active slot
    double* X; double* G; double* D;        // [R][n]: iterate, its gradient, search direction
    double* S; double* Y;                   // [R][kLbfgsM][n]: history ring
    double* trial;           // [A][n]: the points the next evaluation is asked for
    const double* g_trial;   // [A][n]: gradient at the trial points
    const double* f_trial;   // [A]
    double* trace;           // optional [.][trace_len]: row owner[r], entry trace_off + (accepted iterations before) = f
    const int32_t* owner;    // [R]
    int64_t trace_len, trace_off;
    int64_t lds_doubles;     // set by launch_lbfgs_feed: dynamic LDS of the launch, in doubles
};
hipError_t launch_lbfgs_trial(const LbfgsArgs& a, int n_active, hipStream_t s);
hipError_t launch_lbfgs_feed(const LbfgsArgs& a, int n_active, hipStream_t s);
// SAEM E-step (Metropolis-Hastings) helper kernels
hipError_t launch_mh_propose(int64_t N, const double* p, const double* z, RngKey key, double proposal_std, double* prop,
                             hipStream_t s);
// the draws themselves (normals[N], uniforms[N] of one step), for reproducing a device-generated chain elsewhere
hipError_t launch_rng_draws(int64_t N, RngKey key, double* normals, double* uniforms, hipStream_t s);
hipError_t launch_mh_accept(const MhArgs& a, hipStream_t s);
// gamma < 1: proposal and the two possible next states as three parameter sets [3][N]; the decision behind their solves
hipError_t launch_mh_blend_candidates(int64_t N, const double* p, const double* z, RngKey key, double proposal_std, double gamma,
                                      double* cand, hipStream_t s);
hipError_t launch_mh_accept_blend(const MhArgs& a, const double* cand, const double* sse, hipStream_t s);
// per-subject 1-D fits (cude_fit_conditional): device-resident search state, all arrays [N]
struct FitArgs {
    int64_t N;
    double* a; double* b; double* c; double* d;   // bracket and the two probes
    double* fc; double* best;                     // best grid value / index (scan), objective at the result (finish)
    const double* sse_c; const double* sse_d;     // per-subject SSE at the probes c and d
    double w, mu;                                 // penalty w (x - mu)^2
    double lower, step, gr;                       // grid = lower + k*step; golden ratio (sqrt(5)-1)/2
    int32_t n_grid;
};
// phase 0: grid scan update (k = grid index, x = its value); 1: bracket; 2: golden step (k = 1 on the last one);
// 3: objective at the result
hipError_t launch_fit(int phase, const FitArgs& a, int k, double x, hipStream_t s);
// several probes per forward launch (cude_common.hip): the grid scan's update over sets [k0, k0 + kn) of one launch; the
// golden section's next `depth` steps as a heap of brackets, 2 (2^depth - 1) probes in cand / sse_sets [set][N]
constexpr int kFitSpecMaxDepth = 4;
hipError_t launch_fit_grid_all(const FitArgs& a, int k0, int kn, const double* values, const double* sse_sets, hipStream_t s);
hipError_t launch_fit_tree(const FitArgs& a, int depth, int resolve, int final, double* cand, const double* sse_sets, hipStream_t s);
// per-subject Newton-type fits (cude_refine_conditional, cude_refine.hip): the rule's constants and the search state, all
// arrays [N] at the subjects' own indices.  The fused kernels read xt (the clamped start is formed from x0) and write the
// six result arrays; the stepped form keeps the whole state on the device between its rounds.
constexpr int kRefineRunning = -1;                // (results: CUDE_REFINE_* of include/cude.h)
struct RefineCfg {
    double lower, upper, xtol, max_step;
    double pw, pc;                                // penalty pw (x - pc)^2
    int32_t max_evals;
};
struct RefineArrays {
    int64_t N;
    const double* x0;                             // starts (not clamped yet)
    double* x; double* F; double* sse; double* info;      // current point, its objective, SSE and information sum
    int32_t* evals; int32_t* status;
    double* g; double* lam; double* xp; double* gp; double* xt;      // stepped form: half gradient, damping, secant pair, trial
    const double* sse_t; const double* score_t; const double* info_t;   // stepped form: the evaluation at xt
};
// The fused form with a replicate dimension (cude_bootstrap_conditional): a grid of blk_count x n_reps workgroups, (x, y)
// fitting subjects 64 (blk_first + x) ... of replicate y on the observations slab + y * slab_stride (the population's own
// layout: obs [T][N] / data [3][T][N]) from RefineArrays::x0, and storing ONLY x and status, at [y * rep_stride + subject].
// A kernel family of its own beside the one-replicate kernels: with these fields in RefineArrays the one-replicate kernels
// compiled to other register counts and spills (profiles/bootstrap.txt), and they are held to what they were.
struct RefineReps {
    const double* slab; int64_t slab_stride, rep_stride, blk_first, blk_count;
    int32_t n_reps;
};
// fused form (fixed-step mode): hipErrorInvalidValue when no kernel is compiled for the shape.  reps: the replicate family.
hipError_t launch_cpep_refine(const NetShape& net, int n_state, const CpepArgs& a, const RefineCfg& k, const RefineArrays& r, hipStream_t s,
                              const RefineReps* reps = nullptr);
hipError_t launch_supp_refine(const NetShape& net, const SuppArgs& a, const RefineCfg& k, const RefineArrays& r, hipStream_t s,
                              const RefineReps* reps = nullptr);
// phase 0 = clamp the starts, 1 = the rule's update behind an evaluation at xt (both: stepped form); 2 = objective at the
// result from the SSE in r.sse (either form)
hipError_t launch_refine_step(int phase, const RefineCfg& k, const RefineArrays& r, hipStream_t s);
// Parametric bootstrap of the per-subject fits (cude_bootstrap_conditional, cude_bootstrap.hip; the numbered rules in
// include/cude.h).  Replicate data of subjects [subj0, subj0 + n_subj): slab[b][r][i] = yhat[r, i] + sigma[i] * s_r * eps, eps
// = what the slab held (host noise, uploaded in place) or the Philox draw of (subject_offset + i, first_rep + b, r); rows of
// t_0 are copied from `pop`.
constexpr int64_t kRngMaxReplicate = (int64_t)1 << 47;     // replicate indices the draws' counter holds (cude_rng.h)
struct BootstrapGenArgs {
    int64_t N, subj0, n_subj;
    int32_t T, n_states, traj_states;             // rows r = s * T + t, s < n_states; yhat(s, t, i) = traj[s + traj_states (t + T i)]
    double scale[3];                              // s_r of state s
    const double* traj; const double* sigma; const double* pop;     // pop: [n_states * T][N], the slab's layout
    double* slab;                                 // [n_reps][n_states * T][N]
    int32_t n_reps, from_noise;                   // from_noise: eps is read from the slab; 0: drawn
    uint64_t seed; int64_t subject_offset, first_rep;
};
hipError_t launch_bootstrap_generate(const BootstrapGenArgs& a, hipStream_t s);
// eps alone: out[b][r][i] (t_0 rows +0.0), the draws launch_bootstrap_generate uses
hipError_t launch_bootstrap_noise(const BootstrapGenArgs& a, double* out, hipStream_t s);
// Rule 5 over reps / status [K][stride] (subject i of the launch at column i, n_subj of them): per subject n_used, the
// sequential mean, the two-pass sd and the order statistics `ranks_dev` of its non-FAILED estimates.  Outputs at the
// subject's index of the launch: order [n_ranks][out_stride], mean, sd, n_used [.] (order null with n_ranks == 0).
struct BootstrapReduceArgs {
    const double* reps; const int32_t* status; int64_t stride, n_subj;
    int32_t K, n_ranks;
    double* order; int64_t out_stride;
    double* mean; double* sd; int32_t* n_used;
};
hipError_t launch_bootstrap_reduce(const BootstrapReduceArgs& a, const int32_t* ranks_dev, hipStream_t s);
// Prediction discrepancies and npde (cude_npde, cude_npde.hip; the numbered rules in include/cude.h).
constexpr int kNpdeMaxRows = kMaxObs - 1;         // R = T - 1
constexpr int32_t kNpdeSingular = 1, kNpdeFew = 2, kNpdeFailedSims = 4, kNpdeBadObs = 8;      // CUDE_NPDE_*
// Rule 2's sets, or (normals_only) the z alone: out[k][i] over all N subjects
struct NpdePlaceArgs {
    int64_t N; int32_t K, normals_only;
    double prior_mean, prior_sd;
    uint64_t seed; int64_t subject_offset, first_rep;
    double* out;                                  // [K][N]
};
hipError_t launch_npde_place(const NpdePlaceArgs& a, hipStream_t s);
// Rule 4 for subjects [subj0, subj0 + n_subj): y[k][r][li] = slab value of (set k, subject li, time r + 1, `state`) +
// (sigma s) eps, and used[k][li] = every row finite.  slab: [K][n_subj][T][NS] (the multi-set dense-output launch's).  eps:
// what y held (host noise, uploaded there) or the Philox draw of (subject_offset + subj0 + li, first_rep + k, r).
// noise_only: y[k][r][li] = eps alone (slab, sigma, used unused).
struct NpdeObserveArgs {
    int64_t subj0, n_subj;
    int32_t K, T, NS, state, from_noise, noise_only;
    double scale;
    const double* slab; const double* sigma;      // sigma: [N] of the population
    double* y; uint8_t* used;                     // [K][T - 1][n_subj], [K][n_subj]
    uint64_t seed; int64_t subject_offset, first_rep;
};
hipError_t launch_npde_observe(const NpdeObserveArgs& a, hipStream_t s);
// Rules 5 ... 9 over y / used of one pass.  obs: the population's row of (state, t_0), [T][N] from there; outputs [R][N]
// (n_used, status [N]) at the population's own subject index, any of them null.  n_failed: incremented per subject with
// SINGULAR, FEW or BAD_OBS.
struct NpdeReduceArgs {
    int64_t N, subj0, n_subj;
    int32_t K, R;
    const double* y; const uint8_t* used; const double* obs; const double* sigma;
    double* pred_mean; double* pred_var; double* pd; double* npde;
    int32_t* below; int32_t* below_decorr; int32_t* n_used; int32_t* status; int32_t* n_failed;
};
hipError_t launch_npde_reduce(const NpdeReduceArgs& a, hipStream_t s);
// Visual predictive check by subject group (cude_vpc, cude_vpc.hip; the numbered rules in include/cude.h).
constexpr int kVpcMaxGroups = 8, kVpcMaxLevels = 8;
constexpr int32_t kVpcNoGroup = 1, kVpcFailedSims = 2, kVpcBadObs = 4;      // CUDE_VPC_*
// bad[i] = 1: a non-finite observation in a row of obs ([T][N] from the row of t_0), or a non-finite sigma[i]
hipError_t launch_vpc_bad_obs(int64_t N, int R, const double* obs, const double* sigma, uint8_t* bad, hipStream_t s);
// Rule 5's left-out simulations of a pass: grp [N] = the stratum a subject counts in (< 0: none), used [K][N]
// (launch_npde_observe's).  sim_bad[k * G + g] = 1 and status[i] |= kVpcFailedSims where a member's simulation is not used.
hipError_t launch_vpc_flag(int64_t N, int K, int G, const int32_t* grp, const uint8_t* used, uint8_t* sim_bad, int32_t* status,
                           hipStream_t s);
// Rule 3 across the n members of ONE group: column (k, r) is y[(k R + r) N + members[j]], j < n; out[((k G + g) R + r) L + l]
// = its quantile at levels[l] (NaN where n == 0 or sim_bad[k * G + g]; sim_bad may be null).  n <= 4096: the sorting tile,
// unless force_select; longer columns: the radix select, one workgroup per column.
struct VpcColumnsArgs {
    const double* y; int64_t N;
    const int32_t* members; int32_t n;
    int32_t K, R, G, g, L;
    const double* levels;                         // [L] on the device
    const uint8_t* sim_bad;                       // [K][G] of this pass, or null
    double* out;                                  // [K][G][R][L] of this pass
};
hipError_t launch_vpc_columns(const VpcColumnsArgs& a, bool force_select, hipStream_t s);
// n_used[g] = the simulations of sim_bad [K][G] that are not flagged
hipError_t launch_vpc_count(int K, int G, const uint8_t* sim_bad, int32_t* n_used, hipStream_t s);
// Rule 6: ci[((g R + r) L + l) C + c] = rule 3 at ci_levels[c] over the n_used[g] used values sim_q[., g, r, l] (NaN where
// n_members[g] == 0 or n_used[g] == 0)
struct VpcIntervalArgs {
    const double* sim_q; const uint8_t* sim_bad; const int32_t* n_used; const int32_t* n_members;
    int32_t K, G, R, L, C;
    const double* ci_levels;                      // [C] on the device
    double* ci;
};
hipError_t launch_vpc_interval(const VpcIntervalArgs& a, hipStream_t s);
// per-subject profile-likelihood intervals (cude_profile_intervals, cude_common.hip): the scan's running state, the ends'
// brackets and the CUDE_CI_* bits of include/cude.h; all arrays [N] unless noted
constexpr int kProfileWaves = 4;                  // waves of a reduction workgroup: the set dimension is split over them
constexpr int kProfileMaxSections = 16;
constexpr int32_t kProfileLowerOpen = 1, kProfileUpperOpen = 2, kProfileDisconnected = 4, kProfileEmpty = 8,
                  kProfileCenterFailed = 16, kProfileBelowCenter = 32;
struct ProfileArgs {
    int64_t N;
    int32_t n_points;
    double pw, pc;                                // penalty pw (x - pc)^2
    const double* values;                         // [n_points]
    double* thr; double* fcen;                    // threshold and objective at the centre; thr null: minimum and argmin only
    double* fmin; int32_t* imin; int32_t* first; int32_t* last; int32_t* cnt;     // running state of the scan
    double* p_fmin; int32_t* p_imin; int32_t* p_first; int32_t* p_last; int32_t* p_cnt;   // [rows][N] of one chunk's reduction
};
struct ProfileEnds {
    double* lo_out; double* lo_in; double* hi_in; double* hi_out;      // out = NaN: no bracket (open, empty, failed)
    double* argmin;
    int32_t* status;
};
// centre objective, threshold (delta_i [N] or null: delta) and the empty running state
hipError_t launch_profile_init(const ProfileArgs& a, const double* center, const double* sse_center, double delta,
                               const double* delta_i, hipStream_t s);
// sets [k0, k0 + kn) of the scan (sse [kn][N]) into the running state; profile_reduce_rows: partial rows it needs
int profile_reduce_rows(int64_t N, int kn);
hipError_t launch_profile_reduce(const ProfileArgs& a, int k0, int kn, const double* sse, hipStream_t s);
hipError_t launch_profile_finish(const ProfileArgs& a, const ProfileEnds& e, hipStream_t s);
// one sectioning round with m interior points per end: resolve = 0 places the 2m candidates [2m][N], 1 moves the brackets
hipError_t launch_profile_round(const ProfileArgs& a, const ProfileEnds& e, int m, int resolve, double* cand, const double* sse,
                                hipStream_t s);
// per-subject best of n_sets objectives (cude_evaluate_conditional_sets, cude_common.hip): sets [k0, k0 + kn) of sse / x
// ([kn][N] each) into the running minimum fmin [N] and its set index imin [N]; F as cude_profile_intervals rule 1
hipError_t launch_best_of_sets(int64_t N, int k0, int kn, const double* sse, const double* x, double pw, double pc, double* fmin,
                               int32_t* imin, hipStream_t s);
// per-subject marginal likelihoods (cude_marginal_likelihood, cude_marginal.hip; the numbered rules in include/cude.h)
constexpr int kMarginalState = 6;                 // M, S0, S1, S2, S3, Q
struct MarginalArgs {
    int64_t N;
    int32_t n_nodes;
    const double* center;                         // [N]
    const double* scale;                          // [N], or null: 1
    const double* nodes; const double* log_weights;     // [n_nodes] (device memory), or both null: device draws
    RngKey key;                                   // draws: key.step = first_step (node k draws at step first_step + k)
    double c_K;                                   // draws: 0.5 log(2 pi) - log(n_nodes)
    double ll_const, inv_2s2;                     // mh_tempered_ll's constants at temperature 1
    double prior_mean, prior_sd, log_prior_sd;    // prior_sd = +Inf: no prior term
    double* state;                                // [kMarginalState][N], kept between the chunks
    int32_t* n_bad;                               // [N], likewise
};
// rows [k0, k0 + kn) of the points x [kn][N] and (draws) of the standard normals z [kn][N]
hipError_t launch_marginal_points(const MarginalArgs& a, int k0, int kn, double* x, double* z, hipStream_t s);
// nodes [k0, k0 + kn) into the running state, in node order; terms: [kn][N] or null; z: the draws' rows or null (the rule's)
hipError_t launch_marginal_accumulate(const MarginalArgs& a, int k0, int kn, const double* sse, const double* x, const double* z,
                                      double* terms, hipStream_t s);
// outputs [N] each (null: not wanted); n_failed (one zeroed int32): subjects without a finite term
hipError_t launch_marginal_finish(const MarginalArgs& a, double* logml, double* post_mean, double* post_var, double* post_sse,
                                  double* ess, int32_t* n_failed, hipStream_t s);
// per-subject network scores (cude_subject_scores, cude_scores.hip; the numbered rules in include/cude.h): the running
// state of the fold, kept in device memory between the launches of a call
struct ScoresArgs {
    int64_t N;
    int32_t P;
    double* s;                                    // [P][N] weighted rows (after the finish: NaN rows of failed subjects, masked)
    double* wsse;                                 // [N] weighted SSE
    int32_t* bad;                                 // [N] sets with weight whose SSE or row was not finite
    int32_t* fail;                                // [N] 1 = failed subject (written by the finish)
};
// sets [k0, k0 + kn) of a call into the state, in set order: rows [kn][P][N] (CpepArgs::lane_rows), sse and w [kn][N]
// (w null: 1); first: the state starts from zero
hipError_t launch_scores_fold(const ScoresArgs& a, int kn, bool first, const double* rows, const double* sse, const double* w,
                              hipStream_t s);
// failures and the parameter mask (null: none) in place; n_failed (one zeroed int32): failed subjects; score_out_dev: the
// table as [N][P] as well, or null
hipError_t launch_scores_finish(const ScoresArgs& a, const double* mask, int32_t* n_failed, double* score_out_dev, hipStream_t s);
// sum [P] and cross [P][P] over the subjects that did not fail (either null: not wanted); partial: scores_cross_partials doubles
size_t scores_cross_partials(int64_t N, int P);
hipError_t launch_scores_cross(const ScoresArgs& a, double* partial, double* sum, double* cross, hipStream_t s);
// output Jacobians and expected information (cude_network_information, cude_jacobian.hip; the numbered rules in
// include/cude.h): the running state of the fold, kept in device memory between the launches of a call.  Live output l (the
// sets of the unit-seeded launches: CpepArgs::unit_seed) is output out_index(l) of the caller's tables.
struct InfoArgs {
    int64_t N;
    int32_t P, n_out, supp;                       // supp: 1 = the suppression model's 3 T outputs, 0 = T c-peptide outputs
    double w[3];                                  // loss weight of state s (c-peptide: w[1] = 1)
    double pw;                                    // penalty weight
    double* b;                                    // [P][N] coupling rows (after the finish: NaN rows of failed subjects)
    double* d;                                    // [N]
    double* t;                                    // [P][N] b_i / sqrt(d_i + pw), zero for failed and flat subjects
    double* jc;                                   // [N][n_out]
    double* qf;                                   // [N][n_out]
    int32_t* bad;                                 // [N] outputs whose SSE, row or jc was not finite
    int32_t* status;                              // [N] bit 1 = failed, bit 2 = flat (written by the finish)
    const double* mask;                           // [P] parameter mask or null
    __host__ __device__ int out_index(int l) const { return supp ? 3 * (1 + (l >> 1)) + 1 + (l & 1) : l + 1; }
    __host__ __device__ double weight(int l) const { return supp ? w[1 + (l & 1)] : w[1]; }
};
hipError_t launch_info_replicate(int64_t N, int kn, const double* src, double* dst, hipStream_t s);
// live outputs [l0, l0 + kn) into the state, in output order: rows [kn][P][N], jc and sse [kn][N]; first: from zero
hipError_t launch_info_fold(const InfoArgs& a, int kn, int l0, bool first, const double* rows, const double* jc, const double* sse,
                            hipStream_t s);
// n_failed: one zeroed int32
hipError_t launch_info_finish(const InfoArgs& a, int32_t* n_failed, hipStream_t s);
// src [kn][P][N] -> dst [N][dst_rows][P], set k at row out_index(l0 + k) - out_index(l0) (l0 < 0: row k)
hipError_t launch_info_transpose(const InfoArgs& a, int kn, int l0, int dst_rows, const double* src, bool apply_mask, double* dst,
                                 hipStream_t s);
// partial (info_cross_partials doubles) += the weighted cross products of the live outputs [l0, l0 + kn) over the subjects
// whose status (null: everybody's) has no failed bit; l0 < 0: one table of weight 1.  Then the blocks' sums -> dst [P][P].
size_t info_cross_partials(int64_t N, int P);
hipError_t launch_info_cross(const InfoArgs& a, int kn, int l0, bool first, const double* rows, const int32_t* status,
                             double* partial, hipStream_t s);
hipError_t launch_info_cross_finish(const InfoArgs& a, const double* partial, double* dst, hipStream_t s);
hipError_t launch_info_schur(int P, const double* gn, const double* x, double* schur, hipStream_t s);
hipError_t launch_info_qform(const InfoArgs& a, int kn, int l0, bool profiled, const double* rows, const double* jc,
                             const double* cov, hipStream_t s);
// exact order statistics and the sequential mean of every (subject, output time) column of a multi-set dense-output slab
// (cude_predictive_bands, cude_predictive.hip).  slab: value of set k, column q at slab[k * set_stride + q * col_stride];
// columns q in [0, n_cols) with q = j + Tc * (subject - first subject of the launch), j the time inside the chunk
constexpr int kPredMaxSets = 4096, kPredMaxRanks = 16;
struct PredictiveArgs {
    const double* slab; int64_t set_stride, col_stride, n_cols;
    int32_t K, Tc, n_ranks;
    int64_t subj0; int32_t t0, n_times;          // position of the launch's first column in the outputs
    double* order; double* mean;                 // [n_ranks x n_times x N], [n_times x N] or nullptr
    uint8_t* bad; int64_t bad_stride;            // bad[subject * bad_stride + k] = 1: set k of the subject held a non-finite value
};
hipError_t launch_predictive_select(const PredictiveArgs& a, const int32_t* ranks_dev, hipStream_t s);
// bad_sets[i] = number of flagged sets of subject i
hipError_t launch_predictive_count(int64_t N, int K, const uint8_t* bad, int32_t* bad_sets, hipStream_t s);
hipError_t launch_fill(int64_t N, double v, double* out, hipStream_t s);
hipError_t launch_fill_rows(int64_t N, int n_rows, const double* values, double* out, hipStream_t s);
// population preparation
hipError_t launch_prepare_cpep(int64_t N, int T, const double* glucose_tn, const double* cpep_tn, const double* age,
                               const uint8_t* t2dm, double* k0, double* k1, double* k2, double* c0, double* dG,
                               hipStream_t s);

}  // namespace cude
