/* cude.h -- C ABI of libcude_hip.so: the MI355X (gfx950) population ensemble ODE solve +
 * discrete adjoint for conditional universal differential equations.
 *
 * This is the drop-in boundary for ONE hot path of Computational-Biology-TUe/conditional-ude:
 * everything Optimization.jl calls as `f(theta, p)` / its gradient while training a cUDE.
 * The reference has no FFI layer (it is pure Julia); each entry point below names the
 * reference function(s) (paths relative to the reference repo root) whose arithmetic it
 * replaces, so a maintainer can bind it with `ccall` (INTEGRATION.md has the Julia stubs).
 *
 * Conventions
 *   - every function returns int32 status: 0 = ok, <0 = error (CUDE_ERR_*); the message is
 *     available from cude_last_error() (thread-local).  No exceptions, no abort().
 *   - fp64 throughout.  The caller owns every host buffer; the library copies on set_* and
 *     never retains host pointers.  All device memory is owned by the context.
 *   - a context is bound to one HIP device and one stream; it is not thread-safe.
 *   - solver failure convention of the reference (src/parameter-estimation.jl:61-64,134-136):
 *     a non-finite trajectory in any subject makes the returned loss +Inf with status 0;
 *     cude_n_failed() tells how many subjects failed.
 *   - discretisation: fixed-step Tsit5, n_steps uniform steps over [t[0], t[T-1]],
 *     observations by the Tsit5 dense-output interpolant (DESIGN.md "numerical contract"); n_steps = 0 selects the
 *     reference's own adaptive Tsit5 (every entry point; gradients = adjoint of the accepted steps).
 */
#ifndef CUDE_H
#define CUDE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CUDE_OK 0
#define CUDE_ERR_ARG (-1)         /* bad argument / size */
#define CUDE_ERR_HIP (-2)         /* HIP runtime error (message has hipGetErrorString) */
#define CUDE_ERR_STATE (-3)       /* call order (e.g. loss before set_population) */
#define CUDE_ERR_UNSUPPORTED (-4) /* network shape / model not compiled in */
#define CUDE_ERR_COMM (-5)        /* RCCL error or librccl not loadable */

#define CUDE_MODEL_CPEP 0 /* c-peptide cUDE: src/c-peptide-models.jl:7-14,86-94,170-194 */
#define CUDE_MODEL_SUPP 1 /* suppression cUDE: suppression/src/suppression_model.jl:88-95 */
/* c-peptide model with the analytic (symbolic-regression) production term instead of the network:
 * production(dG, k) = dG >= 0 ? p0*dG/(dG + k) : 0  with p0 = 1.78 in the reference
 * (c-peptide/03-symreg.jl:37-40 via CPeptideODEModel / analytic_production, src/c-peptide-models.jl:68-75,
 * 118-142; src/saem-symreg.jl:23-29 writes the same term).  The shared parameter vector is [p0] (P = 1,
 * cude_n_params(.,0,0)); the per-subject conditional parameter is k.  Population data, loss, gradient,
 * multi-start, Metropolis E-step, Adam and sharding are those of CUDE_MODEL_CPEP. */
#define CUDE_MODEL_CPEP_SYM 2

/* how the per-subject conditional parameter enters the symbolic model (cude_config.cond_space) */
#define CUDE_COND_LOG 0 /* k = exp(conditional): the cUDE convention; km_pop*exp(eta) of saem-symreg.jl:57-59 */
#define CUDE_COND_RAW 1 /* k = conditional: the box-constrained fit of 03-symreg.jl:99-106 (p.ode[1] in [0,1000]) */

#define CUDE_UNIQUE_ID_BYTES 128
#define CUDE_XCHG_HANDLE_BYTES 128 /* a rank's exchange mailbox, as cude_xchg_export describes it to its peers */
#define CUDE_XCHG_MAX_RANKS 16    /* ranks of one node (the exchange writes into peers' memory over xGMI) */

typedef struct cude_ctx cude_ctx;

/* Replaces the per-script constants + `chain(width, depth, tanh; input_dims)`
 * (src/neural-network.jl:105-107; suppression_model.jl:78-85) that fix the model shape. */
typedef struct cude_config {
    int32_t model;    /* CUDE_MODEL_* */
    int32_t n_state;  /* CPEP: 2, or 3 = +cumulative-secretion quadrature state (zero loss weight); SUPP: 3 */
    int32_t nn_in;    /* CPEP: 2 = [dG, exp(beta)], 3 = [dG, exp(beta), age] (covariate model,
                         src/c-peptide-models.jl:96-104); SUPP: 4 = [u1,u2,u3,exp(theta)] */
    int32_t nn_width; /* hidden width (0 for CUDE_MODEL_CPEP_SYM) */
    int32_t nn_depth; /* number of hidden layers (tanh unless cude_set_option says otherwise); output layer: 1 unit, softplus
                         unless cude_set_option says otherwise (0 for CPEP_SYM) */
    int32_t n_steps;  /* fixed Tsit5 steps over the time span; 0 = ADAPTIVE Tsit5 as the reference runs it
                         (OrdinaryDiffEq defaults abstol 1e-6 / reltol 1e-3, PI controller, cude_set_tolerances), in
                         every entry point.  Gradients in this mode are those of the accepted step sequence taken as
                         fixed arithmetic -- what AutoForwardDiff through `solve` yields, dt carrying no partials
                         (src/parameter-estimation.jl:165, suppression_model.jl:155); CPEP: n_state = 2 only */
    int32_t device;   /* HIP device ordinal */
    int32_t cond_space; /* CUDE_COND_*; must be CUDE_COND_LOG (0) for the network models */
    double lambda;    /* L2 weight on the network parameters (suppression_loss :128); 0 for CPEP */
} cude_config;

const char* cude_last_error(void);
int32_t cude_device_count(int32_t* count);
/* Number of network parameters for a shape: SimpleChains layout, per layer
 * [vec_colmajor(W out x in); b] (src/neural-network.jl:52-56).  width = depth = 0 names the analytic production
 * model (CUDE_MODEL_CPEP_SYM): 1 shared parameter. */
int32_t cude_n_params(int32_t nn_in, int32_t nn_width, int32_t nn_depth);

/* Any (nn_in, nn_width, nn_depth) is accepted for the network models: shapes a tuned kernel is compiled for (24 c-peptide
 * + 16 suppression shapes, widths <= 8) run on it, every other on the fallback kernel of cude_set_network below. */
int32_t cude_create(const cude_config* cfg, cude_ctx** out);
/* The general form of `chain(widths, activation_functions; input_dims, output_dims = 1, output_activation)`,
 * src/neural-network.jl:42-58 (the docstring's example: chain([10, 20, 30], [tanh, relu, softplus]; input_dims = 4)):
 * n_hidden layer widths and n_hidden + 1 activation codes, one per hidden layer and the output layer's last.  Replaces the
 * network of the context (cfg.nn_in stays; call it after cude_create and before the population is uploaded); the parameter
 * vector is SimpleChains' [vec_colmajor(W); b] per layer and cude_network_info tells its length.  One width, tanh in every
 * hidden layer, softplus at the output and a tuned kernel compiled for it: that kernel; anything else runs on the
 * fallback kernel (csrc/cude_generic.hip: run-time shape, weights staged once per workgroup in LDS, one lane per
 * subject, fixed-step and adaptive, forward and adjoint, both network models) -- every entry point of this header works
 * on it except cude_adaptive_regroup; built for generality, not for speed.  CUDE_ERR_UNSUPPORTED only when the weights
 * and one activation column per lane exceed the 160 KB of LDS of a workgroup (sum of widths around 250) or for more
 * than 8 hidden layers. */
#define CUDE_ACT_TANH 0
#define CUDE_ACT_RELU 1
#define CUDE_ACT_SIGMOID 2
#define CUDE_ACT_SOFTPLUS 3
#define CUDE_ACT_IDENTITY 4
int32_t cude_set_network(cude_ctx* ctx, int32_t n_hidden, const int32_t* widths, const int32_t* activations);
/* Length of the context's shared parameter vector and whether its network runs on the fallback kernel (1) or a tuned one (0). */
int32_t cude_network_info(cude_ctx* ctx, int32_t* n_params, int32_t* fallback_kernel);
int32_t cude_destroy(cude_ctx* ctx);
/* Tolerances of the adaptive mode (cude_config.n_steps = 0): `solve(...; abstol, reltol)`; the defaults 1e-6 / 1e-3
 * are OrdinaryDiffEq's, which every solve call of the reference uses (src/parameter-estimation.jl:59, src/saem.jl:52,
 * suppression/src/suppression_model.jl:113,123). */
int32_t cude_set_tolerances(cude_ctx* ctx, double abstol, double reltol);
/* Adaptive mode: the accepted steps (t_n, dt_n) `subject` took in the last gradient evaluation of the context's own
 * parameters (cude_loss_grad, cude_loss_grad_partial, cude_adam_step ...) -- `sol.t` of the reference's solve.
 * *n_steps = number of accepted steps; at most `cap` of them are written to t_out / dt_out (either may be NULL).
 * CUDE_ERR_STATE before the first such evaluation, outside the adaptive mode, and when any other adaptive launch
 * (cude_forward, a fit, a likelihood profile, a multi-set evaluation, a re-ordering) has run on the context since: those
 * overwrite the step counts the tape is read with. */
int32_t cude_adaptive_steps(cude_ctx* ctx, int64_t subject, int32_t cap, double* t_out, double* dt_out, int32_t* n_steps);
/* Adaptive mode, large populations: order the launch by accepted-step count.  A wave's 64 lanes run until the slowest of
 * them has finished, and subjects differ in how many steps the controller grants them (8 ... 23 on the c-peptide data).
 * Every adaptive launch (forward or gradient) leaves each subject's accepted-step count behind; this call sorts the
 * launch by them (stable, most steps first) so that the lanes of a wave finish together: lane k of the next launches
 * works on the subject that came k-th, inputs are gathered through the permutation, the tape stays in lane order
 * (coalesced), every per-subject output lands at its subject's own index.  Per-subject results are unchanged bit for
 * bit; the shared gradient is summed in the new order (rounding).  spread_* (optional): mean over the waves of (max -
 * min accepted steps within the wave), before and after.  Until the next gradient evaluation cude_adaptive_steps returns
 * CUDE_ERR_STATE (the tape on the device is in the old order).  A new population resets the order.
 * WHO CALLS IT BY ITSELF (populations of >= 8192 subjects; option "auto_regroup" = 0 / CUDE_NO_AUTO_REGROUP=1 turns all
 * of this off): cude_adam_run -- after its 1st, 200th, 400th ... iteration on the population, counted over calls, so
 * that adam_run(400) and 2 x adam_run(200) produce the same bits (single cude_adam_step calls never re-order);
 * cude_multistart_loss_grad / cude_train_restarts -- at the first call that finds counts, then after every 200th
 * evaluation; cude_fit_conditional -- after its first probe.  A caller who needs one summation order across entry
 * points switches the option off and calls this function where it wants the order to change.  (No reference line:
 * the reference solves its subjects one after the other, suppression_model.jl:113,123; parameter-estimation.jl:126-140.) */
int32_t cude_adaptive_regroup(cude_ctx* ctx, int32_t* spread_before, int32_t* spread_after);

/* --- population (replaces the CPeptideConditionalUDEModel constructor loop,
 * src/c-peptide-models.jl:170-194 incl. van_cauter_parameters :30-42, u0, tspan and the
 * LinearInterpolation of glucose :181; c-peptide/02-conditional.jl:26-28).
 * glucose / cpeptide are N x T matrices addressed as base[i*ld_subject + t*ld_time]
 * (Julia column-major N x T: ld_subject = 1, ld_time = N; numpy C-order: ld_subject = T, ld_time = 1).
 * age[N], t2dm[N] (0/1).  timepoints[T] are shared by all subjects and are also the glucose knots.
 * If a communicator is attached (cude_comm_init) the global subject count is all-reduced here. */
int32_t cude_set_population_cpep(cude_ctx* ctx, int64_t n_subjects, int32_t n_obs, const double* timepoints,
                                 const double* glucose, const double* cpeptide, int64_t ld_subject,
                                 int64_t ld_time, const double* age, const uint8_t* t2dm);

/* suppression model population: data is the Julia array individual_data[3 x T x N] in
 * column-major order (data[s + 3*(t + T*i)]); u0 = data[:,1,:]; scale = mean_i max_t data
 * (suppression_model.jl:119,126). */
int32_t cude_set_population_supp(cude_ctx* ctx, int64_t n_subjects, int32_t n_obs, const double* timepoints,
                                 const double* data);

/* theta = ComponentArray(neural = nn[P], conditional = cond[N]) (parameter-estimation.jl:354-357).
 * Either pointer may be NULL to leave that part unchanged. */
int32_t cude_set_params(cude_ctx* ctx, const double* nn, const double* cond);
int32_t cude_get_params(cude_ctx* ctx, double* nn, double* cond);

/* Forward-only population loss: `loss(theta, (models, timepoints, data))`
 * (src/parameter-estimation.jl:126-140, per-subject :56-68) / `suppression_loss` without AD
 * (suppression_model.jl:117-130) / `simul` (:107-115).
 * per_subject_sse[N] (optional) is the un-normalised SSE of each subject (the quantity
 * loss_sigma :70-75 and individual_log_likelihood saem.jl:55-66 are built from).
 * traj (optional) receives the interpolated states as [n_state x T x N] column-major
 * (Julia Array(sol) layout of simul). */
int32_t cude_forward(cude_ctx* ctx, double* loss, double* per_subject_sse, double* traj);

/* Dense output: the states of every subject at n_times arbitrary, non-decreasing times inside [t[0], t[T-1]] (Tsit5
 * interpolant of the same solve), at the context's current parameters (parameter set 0).  Replaces
 * `simulate(p_neural, p_individual, individual, network; timepoints = t0:0.1:tend)` (src/saem.jl:31-53, called with
 * dense grids at c-peptide/06-saem.jl:221-240) and `solve(model.problem, p=..., saveat=sol_timepoints)` of the
 * model-fit figures (c-peptide/02-conditional.jl, 03-symreg.jl:113), and -- suppression model: u0 from the data's first
 * column, n_state = 3 -- `simul(p, prob, individual_data, timepoints)` at save times other than the data's
 * (suppression/src/suppression_model.jl:107-115, as suppression/figures.jl:66-74 calls it on range(0, 30, length = 100)).
 * Fixed-step or adaptive as the context is: the adaptive solve takes the same steps as cude_forward's (the output times are
 * `saveat`, not `tstops`).  traj receives [n_state x n_times x N] column-major.  A failed subject leaves the others
 * unaffected: an adaptive solve that fails (non-finite error estimate, step limit) leaves NaN at every output time it
 * did not reach, both models; a suppression subject with a non-finite input (theta, u0, a network parameter) gets NaN
 * at every output time (as the oracle's adaptive solve reports it); c-peptide values are otherwise what the
 * arithmetic gives, as before. */
int32_t cude_simulate(cude_ctx* ctx, int32_t n_times, const double* times, double* traj);

/* Per-subject output sensitivities: the derivative of every subject's trajectory with respect to its OWN conditional
 * parameter, by a tangent-linear (forward-mode) solve next to the solve itself -- what every solve of the reference carries
 * under ForwardDiff (sensealg = ForwardDiffSensitivity(), src/parameter-estimation.jl:59; AutoForwardDiff() through
 * `solve`, src/parameter-estimation.jl:165,370 and suppression/src/suppression_model.jl:155), restricted to the direction
 * d/d(conditional_i).  All four outputs are optional; the context's current parameters are used.
 *   sens  [n_state x T x N] column-major (cude_forward's traj layout): d u_s(t_j) / d cond_i at the data's time points;
 *         column t_0 is exactly 0 (u0 depends on no parameter)
 *   info  [N]  sum over the observed outputs of (w * d yhat / d cond)^2 in the loss's own weighting -- c-peptide models:
 *         state 1, w = 1; suppression model: all three states, w = 1 / scale_s.  The Fisher information of cond_i is
 *         info / sigma^2; an unidentifiable subject (constant glucose) has info = 0
 *   score [N]  sum of w^2 (yhat - y) d yhat / d cond = (1/2) d SSE_i / d cond_i; against cude_loss_grad:
 *         g_cond_i = 2 * score_i / n_global
 *   sse   [N]  cude_forward's per_subject_sse
 * The derivative is with respect to the parameter AS STORED: log-space beta / theta (the chain factor exp(beta) is
 * included), or k itself where cude_config.cond_space is CUDE_COND_RAW.  Adaptive mode: step control reads the solve's
 * own error estimate only, so the accepted steps are cude_forward's and the result is the derivative of the
 * accepted-step map -- the adaptive gradient's convention (OrdinaryDiffEq's norm under duals, which also weighs the
 * partials, is not reproduced); the steps are left where cude_adaptive_steps reads them.  A subject with a non-finite
 * parameter or a failed adaptive solve gets NaN in all its outputs and is counted by cude_n_failed (this rank's
 * subjects); the others are unaffected.  CUDE_ERR_UNSUPPORTED for a network on the fallback kernel (cude_set_network). */
int32_t cude_sensitivity(cude_ctx* ctx, double* sens, double* info, double* score, double* sse);

/* Exact per-subject curvature: the SECOND derivative of every subject's trajectory with respect to its own conditional
 * parameter, by an order-2 forward-mode solve (u, du/dcond and d2u/dcond2 carried together through network, step and
 * interpolant), and with it the true curvature of the subject's objective, of which cude_sensitivity's info is the
 * Gauss-Newton part -- what ForwardDiff.hessian of the per-subject objective of src/parameter-estimation.jl:165,370 /
 * suppression/src/suppression_model.jl:155 gives.  It is the exact second derivative of the discrete map (every stage,
 * the FSAL carry, the dense-output weights), not a discretisation of a second-order sensitivity equation.  All five
 * outputs are optional, at least one must be given; the context's current parameters are used and left untouched.
 *   1. sens2 [n_state x T x N] column-major (cude_forward's traj layout): d^2 u_s(t_j) / d cond_i^2 at the data's time
 *      points.  Column t_0 is exactly 0 (u0 depends on no parameter); suppression state 1 is exactly 0.
 *   2. curv [N] = sum over the observed outputs of w^2 [(d yhat / d cond)^2 + (yhat - y) d^2 yhat / d cond^2]
 *      = (1/2) d^2 SSE_i / d cond_i^2, in cude_sensitivity's weighting: c-peptide models state 1 with w = 1, suppression
 *      model all three states with w = 1 / scale_s.  The observed information of cond_i is curv / sigma^2; it may be <= 0
 *      (a saddle or a maximum of the objective, which info >= 0 can never show).
 *   3. info, score and sse are as cude_sensitivity defines them.  Always curv - info = sum w^2 (yhat - y) d^2 yhat / d cond^2.
 *   4. Derivatives are with respect to the parameter AS STORED: log space includes the chain factor at both orders
 *      (d^2/d beta^2 = k^2 d^2/dk^2 + k d/dk), CUDE_COND_RAW takes k itself.  Adaptive mode: step control reads the
 *      solve's own error estimate only, so the accepted steps are cude_forward's and the result is the second derivative
 *      of the accepted-step map (cude_sensitivity's convention); the steps are left where cude_adaptive_steps reads them.
 *   5. Failures are cude_sensitivity's: a subject with a non-finite input or a failed adaptive solve gets NaN in all its
 *      outputs and is counted by cude_n_failed (this rank's subjects); the others are unaffected.
 *   6. CUDE_ERR_UNSUPPORTED for a network on the fallback kernel (cude_set_network) and for a general-activation network
 *      in adaptive mode; CUDE_ERR_STATE without population or parameters, and under stream capture; CUDE_ERR_ARG with no
 *      output.  A sharded population needs no exchange: every rank's subjects are its own. */
int32_t cude_curvature(cude_ctx* ctx, double* sens2, double* curv, double* info, double* score, double* sse);

/* Multi-start screening: forward-only loss of n_sets candidate parameter sets over the resident
 * population in one launch (first phase of `train`, src/parameter-estimation.jl:351-366;
 * fit_suppression_model suppression_model.jl:135; c-peptide/06-saem.jl:41-42).
 * nn_sets[n_sets][P], cond_sets[n_sets][N] row-major; losses[n_sets] (+Inf for a set with a failed subject).
 * Does not touch the context's current parameters. */
int32_t cude_multistart_forward(cude_ctx* ctx, int32_t n_sets, const double* nn_sets, const double* cond_sets,
                                double* losses);

/* The whole screening phase with the selection on the device: `losses_initial = [loss(p, ...) for p in initials]` followed
 * by `partialsortperm(losses_initial, 1:selected_initials)` (src/parameter-estimation.jl:359-372; suppression_model.jl:
 * 135-145; c-peptide/06-saem.jl:41-45).  Candidates are STREAMED: `gen` is asked for one chunk at a time (candidates
 * first ... first+count-1 as rows nn_sets[count][P], cond_sets[count][N]; return < 0 to abort), so the host never holds
 * the 25 000 x (P + N) candidate table; each chunk is evaluated in one multi-start launch, its losses stay on the device
 * and are merged into a running top-n_keep (ties broken by the lower candidate index, as partialsortperm does), whose
 * parameter sets are kept on the device as well.  Out: index_out / loss_out [n_keep] in increasing order of loss, and
 * the selected parameter sets nn_out[n_keep][P], cond_out[n_keep][N] -- ready for cude_train_restarts. */
typedef int32_t (*cude_candidate_fn)(int64_t first, int32_t count, double* nn_sets, double* cond_sets, void* user);
int32_t cude_screen_candidates(cude_ctx* ctx, int64_t n_candidates, int32_t n_keep, cude_candidate_fn gen, void* user,
                               int64_t* index_out, double* loss_out, double* nn_out, double* cond_out);

/* Restarts trained side by side: loss AND gradient of n_sets independent parameter sets over the resident
 * population in one launch (the grid's second dimension is the set).  The reference trains its selected
 * initial guesses one after the other (`for p in initials[selected] ... _optimize(...)`,
 * src/parameter-estimation.jl:372-383; suppression_model.jl:140-170), each a serial chain of thousands of
 * loss+gradient evaluations over a few dozen subjects -- one wave of work per evaluation; evaluating all restarts'
 * current points together turns that latency-bound loop into a throughput-bound one.
 * nn_sets[n_sets][P], cond_sets[n_sets][N] row-major in; losses[n_sets] (+Inf for a set with a failed subject,
 * L2 term included), g_nn_sets[n_sets][P], g_cond_sets[n_sets][N] out -- exactly what cude_loss_grad returns for
 * each set.  Does not touch the context's current parameters. */
int32_t cude_multistart_loss_grad(cude_ctx* ctx, int32_t n_sets, const double* nn_sets, const double* cond_sets,
                                  double* losses, double* g_nn_sets, double* g_cond_sets);

/* The second half of `train` (src/parameter-estimation.jl:368-383; fit_suppression_model suppression_model.jl:140-170)
 * for n_sets selected initial guesses SIDE BY SIDE: `adam_iters` iterations of Optimisers.Adam(learning_rate), then
 * up to `lbfgs_iters` iterations of Optim's L-BFGS (m = 10) with LineSearches.BackTracking -- every optimiser
 * iteration evaluates all restarts' current points with one cude_multistart_loss_grad launch; each restart follows
 * the path it would follow alone.  A restart whose loss becomes non-finite during Adam is dropped (objective +Inf),
 * as the reference skips a failed optimisation.  In: nn_sets[n_sets][P], cond_sets[n_sets][N]; out: the trained
 * nn_out / cond_out (same layout) and objective_out[n_sets] (`OptimizationSolution.objective`); loss_trace (optional,
 * [n_sets][adam_iters + lbfgs_iters], NaN where a run had already stopped) receives what the reference's callbacks
 * collect: the loss of every Adam iteration, then the loss after every successful L-BFGS iteration.  On a sharded
 * population (cude_comm_init) cond_sets / cond_out hold this rank's subjects; losses and network gradients are
 * all-reduced inside the launch sequence and the conditional part of every L-BFGS inner product is summed over the
 * ranks, so all ranks return the same networks and objectives.  The optimiser
 * bookkeeping runs on the host (vectors of P+N doubles); every loss and gradient comes from the device. */
int32_t cude_train_restarts(cude_ctx* ctx, int32_t n_sets, const double* nn_sets, const double* cond_sets,
                            int32_t adam_iters, double learning_rate, int32_t lbfgs_iters, double* nn_out,
                            double* cond_out, double* objective_out, double* loss_trace);

/* The same L-BFGS + BackTracking for any objective (host only, needs no GPU): `Optimization.solve(prob,
 * LBFGS(linesearch = BackTracking()), maxiters)` with Optim.jl's defaults (memory 10, g_tol 1e-8, c_1 1e-4,
 * rho in [0.1, 0.5], cubic interpolation).  fn fills *f and g[n] at x and returns >= 0 (a non-finite f is a failed
 * solve: the line search backs away from it).  iterations / f_calls / converged may be NULL. */
typedef int32_t (*cude_objective_fn)(const double* x, int32_t n, double* f, double* g, void* user);
int32_t cude_lbfgs_minimize(int32_t n, const double* x0, int32_t maxiters, cude_objective_fn fn, void* user,
                            double* x_out, double* f_out, int32_t* iterations, int32_t* f_calls, int32_t* converged);

/* The same optimiser for a SHARDED vector: x = [shared (n_shared entries, replicated on every rank); local (this
 * rank's n - n_shared conditional parameters)].  fn returns the GLOBAL f and this rank's gradient entries; `reduce`
 * sums (op 0) or takes the maximum (op 1) of `count` doubles over all ranks in place (MPI.Allreduce!, gloo, ...) and
 * returns >= 0.  Every inner product / max-norm of the L-BFGS recursion takes its local part through `reduce`, so all
 * ranks walk the same iterates as one process holding the whole vector would (up to the summation order of the inner
 * products).  This is the second stage of `_optimize` (src/parameter-estimation.jl:179-180) on a population sharded
 * over GPUs; cude_train_restarts does the same internally over its RCCL communicator. */
typedef int32_t (*cude_reduce_fn)(double* values, int32_t count, int32_t op, void* user);
int32_t cude_lbfgs_minimize_sharded(int32_t n, int32_t n_shared, const double* x0, int32_t maxiters,
                                    cude_objective_fn fn, cude_reduce_fn reduce, void* user, double* x_out,
                                    double* f_out, int32_t* iterations, int32_t* f_calls, int32_t* converged);

/* Likelihood profiles of ALL subjects in one launch: sse_out[n_points][N] (row-major) = SSE_i(values[k]) with the
 * shared parameters frozen -- the grid's second dimension is the scan value.  Replaces
 * `likelihood_profile(beta, nn, model, timepoints, data, lower, upper, sigma; steps)` (src/likelihood-profiles.jl:4-17:
 * `loss_values = [loss(b, (model, ...)) for b in range(lower, upper, length = steps)]`, called per subject with
 * 1000-10000 points at c-peptide/02-conditional.jl:186-188); the profile is sse / (2 sigma^2). */
int32_t cude_profile_conditional(cude_ctx* ctx, int32_t n_points, const double* values, double* sse_out);

/* Per-subject fits of the conditional parameter with the shared parameters frozen, for all subjects at once:
 * every subject i minimises  SSE_i(x) + penalty_weight * (x - penalty_center)^2  over [lower, upper] by a coarse scan
 * of n_grid points followed by n_iters golden-section steps inside the best bracket; the whole search is queued on
 * the stream (one forward launch per probe, search state on the device, one synchronisation at the end).
 * Replaces the per-subject loops  `for (i, model) in enumerate(models) ... Optimization.solve(..., LBFGS, Fminbox)`:
 *   train(models, timepoints, data, neural_network_parameters) / train_with_sigma   src/parameter-estimation.jl:272-307
 *   evaluate_model                                                                   :406-433
 *   validate_suppression_model (loss separates per subject for a frozen network)     suppression_model.jl:179-222
 *   the (k, sigma) fits of the symbolic model                                        c-peptide/03-symreg.jl:94-106
 *   MAP (penalty_weight = sigma^2/Omega^2, penalty_center = prior mean) and MLE      c-peptide/06-saem.jl:114-126
 * (for fixed x the sigma of the reference's 2-parameter objectives has the closed form sigma^2 = SSE/n).
 * cond_out[N]; objective_out[N] and sse_out[N] optional.  Uses the context's current shared parameters and leaves
 * its conditional parameters untouched. */
int32_t cude_fit_conditional(cude_ctx* ctx, double lower, double upper, int32_t n_grid, int32_t n_iters,
                             double penalty_weight, double penalty_center, double* cond_out, double* objective_out,
                             double* sse_out);

/* The same per-subject problems by a LOCAL, gradient-based method from a given start -- what the reference's own solver
 * is (`LBFGS` inside `Fminbox` from `initial_beta`, under ForwardDiff: src/parameter-estimation.jl:272-307, :406-433;
 * suppression_model.jl:179-222; c-peptide/03-symreg.jl:94-106; `compute_individual_maps`, src/saem.jl:74-84).  Subject i
 * minimises  F(x) = SSE_i(x) + penalty_weight * (x - penalty_center)^2  over [lower, upper] from x0_i by a damped
 * Newton-type iteration whose every evaluation is one tangent-linear solve (cude_sensitivity's sse, score, info):
 * g = score + pw (x - pc), Hgn = info + pw.
 *   1. x = clamp(x0, lower, upper); evaluate; lambda = 1e-3; no secant pair yet.  Non-finite F: FAILED.
 *   2. c = (g - gp) / (x - xp) over the secant pair (xp, gp); H = c if finite and > 0, else Hgn.  Not H > 0: FLAT.
 *   3. d = clamp(-g / (H (1 + lambda)), +-max_step); xt = clamp(x + d, lower, upper).
 *   4. |xt - x| <= xtol (1 + |x|): AT_BOUND if xt is a bound, else CONVERGED.
 *   5. evaluate at xt; accept iff F(xt) is finite and < F.  Accept: (xp, gp) <- (x, g), move to xt, lambda <-
 *      max(lambda / 10, 1e-12).  Reject: (xp, gp) <- (xt, g(xt)) if F(xt) was finite; lambda <- 10 lambda.
 *   6. evals == max_evals: MAX_EVALS (also right after step 1 when max_evals == 1); otherwise back to 2.
 * Fixed-step mode: ONE launch -- a lane iterates its subject until it stops, a wave retires with its slowest lane
 * (option "refine_fused" = 0: one tangent launch + one update launch per evaluation instead, which is also what the
 * adaptive mode always runs; all max_evals rounds are queued, one synchronisation at the end).
 * xtol: the acceptance test of step 5 compares two objective values, so steps shorter than the width over which the SSE is
 * flat to rounding (~1e-7 in x for the reference's problems) are accepted or rejected by rounding noise; the mirrors'
 * default is 1e-7, where the result is reproducible to ~1e-14 under the tangent kernels' accepted error.
 * x0 [N], or NULL = the context's conditional parameters.  Outputs, all [N], all optional but cond_out: the point
 * reached, its objective, its SSE, cude_sensitivity's info at it, the number of evaluations and the CUDE_REFINE_* status.
 * sse_out is cude_forward's own number at cond_out (one forward launch behind the iteration, as cude_fit_conditional's)
 * and objective_out = sse_out + penalty; the tangent solve's SSE, which the iteration compares, agrees with it to rounding.
 * A FAILED subject returns its clamped start and objective +Inf, does not disturb the others and is counted by
 * cude_n_failed.  Uses the context's shared parameters, leaves its conditional parameters untouched.  Adaptive mode:
 * cude_adaptive_steps refuses afterwards (the last solve was of a trial point).  CUDE_ERR_UNSUPPORTED for a network on
 * the fallback kernel (cude_set_network), CUDE_ERR_STATE under stream capture. */
#define CUDE_REFINE_CONVERGED 0
#define CUDE_REFINE_AT_BOUND 1
#define CUDE_REFINE_MAX_EVALS 2
#define CUDE_REFINE_FLAT 3
#define CUDE_REFINE_FAILED 4
int32_t cude_refine_conditional(cude_ctx* ctx, const double* x0, double lower, double upper, int32_t max_evals,
                                double xtol, double max_step, double penalty_weight, double penalty_center,
                                double* cond_out, double* objective_out, double* sse_out, double* info_out,
                                int32_t* evals_out, int32_t* status_out);

/* Parametric bootstrap of those per-subject fits, on the device: n_reps times per subject, noisy observations are simulated
 * from the fitted model and the conditional parameter is fitted to them again -- the reference's own way of validating an
 * estimate (the noisy data of suppression/src/suppression_model.jl:39-63, refitted as :179-222), here with the replicate as a
 * launch dimension instead of a host loop of uploads and cude_refine_conditional calls.  The host receives per-subject
 * summaries (and the replicate estimates if it asks), never a replicate's data.
 *   1. Centre and prediction: center [N], NULL = the context's conditional parameters.  yhat = the trajectory cude_forward
 *      returns at `center` with the context's shared parameters (the same launch; adaptive mode: its accepted steps).
 *   2. Replicate data: y*[b, r, i] = yhat[r, i] + (sigma[i] s_r) eps[b, r, i] over the residual rows r of the population's own
 *      layout, every operation rounded on its own (no fma).  C-peptide models: the T rows of state 1, s = 1.  Suppression
 *      model: 3 T rows in [3][T][N] order, s = the state's cude_get_scale value; the loss weights stay the population's.
 *      The row(s) of t_0 are the population's own data, never drawn: they are the initial state and their residual is zero.
 *   3. Noise: eps = noise[(b rows + r) N + i] ([n_reps][rows][N]; entries of t_0 rows are ignored), or with noise == NULL
 *      the context's Philox stream (cude_set_rng): key = seed, counter = (global subject, first_rep + b, row) in a block kind
 *      of its own, Box-Muller as the Metropolis draws.  A draw depends on nothing else: identical under any chunking and any
 *      sharding (cude_set_rng's subject_offset).  The context keeps no position: first_rep is the caller's (0 <= first_rep,
 *      first_rep + n_reps <= 2^47).  cude_bootstrap_noise returns exactly the draws such a call uses ([n_reps][rows][N], +0.0
 *      in the t_0 rows).
 *   4. Fits: replicate b of subject i runs cude_refine_conditional's rule (above, steps 1-6, the same device statement) from
 *      x0 = center_i on the replicate's data, with the same box, max_evals, xtol, max_step and penalty.  reps_out and
 *      status_out ([n_reps][N], optional): the points reached and their CUDE_REFINE_* status.  No forward launch follows the
 *      iteration: objectives, SSEs and evaluation counts are not reported.
 *   5. Summaries per subject over its non-FAILED replicates, in replicate order: n_used_out[i] = their count; mean_out[i] =
 *      (((x_0 + x_1) + x_2) + ...) / n_used; sd_out[i] = sqrt(sum (x_b - mean)^2 / (n_used - 1)), a second pass, NaN for
 *      n_used < 2; order_out[r N + i] ([n_ranks][N]) = the ranks[r]-th smallest (0-based) of the non-FAILED estimates -- a
 *      selection: one of the replicate estimates, bit for bit -- and NaN where ranks[r] >= n_used.  ranks strictly increasing
 *      inside [0, n_reps); 0 <= n_ranks <= 16, order_out exactly when n_ranks > 0; at least one output.  mean, sd and order
 *      are NaN with n_used == 0.  The reduction runs over all replicates of a subject at once: every output is bit-identical
 *      for every chunking.
 *   6. CUDE_ERR_ARG for a negative or non-finite sigma entry, for the box, step, penalty and rank errors of
 *      cude_refine_conditional / cude_predictive_bands, and for n_reps outside [1, 4096].  A non-finite center_i fails that
 *      subject alone: all its statuses FAILED, n_used 0, its summaries NaN; cude_n_failed afterwards counts the subjects
 *      with a FAILED replicate.  The caller's noise is not screened: a non-finite entry outside the t_0 rows fails its
 *      replicate of its subject alone (that fit's first objective is non-finite), which rule 5 then leaves out.
 *   7. CUDE_ERR_UNSUPPORTED for a network on the fallback kernel (cude_set_network), CUDE_ERR_STATE under stream capture.
 *   8. Uses the context's shared parameters, leaves its conditional parameters untouched.  Adaptive mode: cude_adaptive_steps
 *      refuses afterwards.
 * Fixed-step mode: the fused kernels of cude_refine_conditional with the replicate in the grid's second dimension -- ONE
 * launch fits a chunk of replicates of all subjects; replicates per launch by ~256 MB of replicate data (option
 * "bootstrap_chunk"), subjects per pass in whole workgroups of 64 by ~1 GB of replicate results (option
 * "bootstrap_subjects"); one stream, no graph.  Adaptive mode and option "refine_fused" = 0: the stepped form, ONE REPLICATE AT
 * A TIME (max_evals tangent launches over the whole population per replicate, all queued) -- slow, n_reps times the cost of
 * a stepped cude_refine_conditional; meant for checking, not for production runs. */
int32_t cude_bootstrap_conditional(cude_ctx* ctx, const double* center, const double* sigma, int64_t first_rep,
                                   int32_t n_reps, const double* noise, double lower, double upper, int32_t max_evals,
                                   double xtol, double max_step, double penalty_weight, double penalty_center,
                                   int32_t n_ranks, const int32_t* ranks, double* order_out, double* mean_out,
                                   double* sd_out, int32_t* n_used_out, double* reps_out, int32_t* status_out);
int32_t cude_bootstrap_noise(cude_ctx* ctx, int64_t first_rep, int32_t n_reps, double* noise_out);

/* Per-subject profile-likelihood intervals with the whole profile kept on the device -- the loop around
 * `find_confidence_intervals(loss_values, loss_minimum, parameter_values; target)` (src/likelihood-profiles.jl:34-59, run
 * for every subject over 1000-10000 profile points at c-peptide/02-conditional.jl:186-188).  The host receives a handful
 * of numbers per subject, never the n_points x N profile.
 *   1. Objective: F_i(x) = SSE_i(x) + pw (x - pc)^2 with the shared parameters frozen at the context's, every operation
 *      rounded on its own: t = x - pc; p = pw (t t); F = SSE + p (no fma contraction: numpy's sse + pw * (x - pc) ** 2
 *      has the same bits; deliberately not cude_fit_conditional's fma form).  A non-finite F is above every threshold.
 *   2. Centre and threshold: center[N] (NULL: the context's conditional parameters) is evaluated once, in one forward
 *      launch (cude_forward's); thr_i = F_i(center_i) + d_i, d_i = delta_per_subject[i] if given, else delta, in SSE
 *      units (the mirrors pass 2 sigma^2 Delta, Delta = 7.16 / 5.24 / chi^2_1(0.95)); d_i >= 0, +Inf allowed.
 *   3. Scan: values[n_points] strictly increasing and finite; every subject at every value as the parameter sets of
 *      cude_profile_conditional's launches (the same SSE bits; option "profile_chunk" = sets per launch).  Every chunk is
 *      reduced on the device into a running per-subject state: the minimum of F and its grid index (strict <: the first
 *      minimum wins; no finite value: index 0, minimum +Inf), the first and the last index with F <= thr, their count.
 *      All of these are exact, so the result depends neither on the chunk size nor on how a chunk is split.
 *   4. Grid result (n_rounds = 0, the reference's answer exactly): lower = values[first], or -Inf if first == 0;
 *      upper = values[last], or +Inf if last == n_points - 1.
 *   5. Refinement: n_rounds rounds (0 ... 64) with n_sections = m interior points per end (1 ... 16; 1 = bisection).  A
 *      closed end has the bracket (out, in) = (values[first - 1], values[first]) / (values[last + 1], values[last]).  A
 *      round evaluates p_j = out + (in - out) j / (m + 1), j = 1 ... m, of both ends in ONE forward launch of 2m sets; the
 *      new `in` is the p_j nearest to `out` with F <= thr (none: `in` stays), the new `out` that point's neighbour on the
 *      out side, so the outermost crossing is kept (as the reference keeps the outermost grid point) and the bracket
 *      shrinks by m + 1 per round.  Open, empty and failed ends ride along at a dummy point and are not written.  The
 *      reported ends are the `in` points: they lie inside the threshold.  All rounds are queued; one synchronisation.
 *   6. Outputs, all [N], all optional, at least one: lower_out, upper_out, argmin_out (= values[index of the minimum]),
 *      min_out, center_objective_out (+Inf for a failed centre), n_inside_out (rule 3's count), status_out (CUDE_CI_*
 *      bits).  With argmin_out / min_out alone the centre solve and the rounds are skipped and nothing is compared to a
 *      threshold.
 *   7. Fixed-step and adaptive mode (adaptive: large populations are re-ordered after the first chunk as in
 *      cude_fit_conditional; cude_adaptive_steps refuses afterwards), both network models, the symbolic model in either
 *      cond_space, the fallback kernel.  A sharded population needs no exchange: every output is per subject.
 *   8. CUDE_ERR_ARG: values not increasing / not finite, n_points < 2, n_sections or n_rounds out of range, a negative
 *      or NaN d_i, no output; CUDE_ERR_STATE: population or shared parameters (or, with center NULL, conditional
 *      parameters) not set, stream capture.
 * Leaves the context's parameters untouched. */
#define CUDE_CI_LOWER_OPEN     1  /* the in-threshold set reaches values[0]: lower = -Inf (reference :55) */
#define CUDE_CI_UPPER_OPEN     2  /* ... reaches values[n_points-1]: upper = +Inf (:56) */
#define CUDE_CI_DISCONNECTED   4  /* grid points above the threshold lie between the outermost ones inside it */
#define CUDE_CI_EMPTY          8  /* no grid point within the threshold: lower = upper = NaN */
#define CUDE_CI_CENTER_FAILED 16  /* objective at the centre not finite: lower = upper = NaN; counted by cude_n_failed */
#define CUDE_CI_BELOW_CENTER  32  /* some grid point has a smaller objective than the centre: the centre is no minimiser */
int32_t cude_profile_intervals(cude_ctx* ctx, int32_t n_points, const double* values, const double* center,
                               double delta, const double* delta_per_subject, double penalty_weight,
                               double penalty_center, int32_t n_rounds, int32_t n_sections,
                               double* lower_out, double* upper_out, double* argmin_out, double* min_out,
                               double* center_objective_out, int32_t* n_inside_out, int32_t* status_out);

/* Posterior-predictive bands from per-subject sample sets, reduced on the device -- the loop that simulates every thinned
 * posterior sample (`test_samples[i][1000:10:end]`, ~200 per individual) on `t0:0.1:tend` and takes quantiles of the
 * curves (c-peptide/06-saem.jl:209-241; the solve is `solve(prob, saveat = ...)` of src/saem.jl:31-53).  The host receives a
 * few curves per subject, never the n_sets x n_times x N sample trajectories.
 *   1. Solve: set k = the context's shared parameters with the conditional vector cond_sets[k] ([n_sets][N] row-major,
 *      the row layout of cude_mh_chain's `samples`), solved exactly as cude_simulate solves the context's own conditional
 *      parameters at `times` (the same kernels, arithmetic and time validation; adaptive mode: the accepted steps of
 *      cude_forward at that vector).  v[k] at (subject i, time j) has the same bits as cude_simulate's state `state` after
 *      cude_set_params(ctx, NULL, cond_sets[k]).
 *   2. Order statistics: order_out[r + n_ranks (j + n_times i)] = the ranks[r]-th smallest (0-based) of v[0 .. n_sets-1] of
 *      column (i, j); ranks strictly increasing, 0 <= ranks[r] < n_sets.  A selection: the result is one of the solve's own
 *      values, bit for bit (rank 0 and rank n_sets - 1: the envelope).  1 <= n_sets <= 4096, 0 <= n_ranks <= 16; order_out
 *      and mean_out may each be NULL, not both.
 *   3. Mean: mean_out[j + n_times i] = (((v[0] + v[1]) + v[2]) + ...) / n_sets -- plain adds in set order, no fma, so the
 *      value does not depend on how the work is split.
 *   4. Non-finite values: a column that holds any non-finite value gets NaN in every order_out entry and in its mean (what
 *      numpy.quantile returns; decided by a test on the values, not by how NaN sorts).  bad_sets_out[i] (optional) = the
 *      number of sets with a non-finite value at any output time of subject i; cude_n_failed afterwards counts the
 *      subjects with bad_sets > 0.  Other subjects are unaffected, bit for bit.  (The values decide: the c-peptide kernels
 *      take the conditional parameter through exp and a table-based tanh, which map a NaN to finite numbers -- there a
 *      NaN sample gives cude_simulate's finite trajectory and marks nothing; the suppression solves carry it through.)
 *   5. Both network models, the symbolic model in either cond_space, fixed-step and adaptive mode, every tuned shape;
 *      state < n_state (suppression state 0 does not depend on the parameter and is allowed).  CUDE_ERR_UNSUPPORTED for a
 *      network on the fallback kernel (cude_set_network), CUDE_ERR_STATE under stream capture, CUDE_ERR_ARG for n_sets,
 *      n_ranks, ranks, state or times out of range.  A sharded population needs no exchange.  Leaves the context's
 *      parameters untouched.  Adaptive mode: cude_adaptive_steps refuses afterwards.
 * The solves are split over subjects first (whole workgroups of 64: no solve is repeated) and over output times only when
 * 64 subjects x n_sets x n_times exceed ~1 GB (every time chunk integrates from t_0 again, as cude_simulate's); options
 * "predictive_subjects" / "predictive_times" force either split, and the result depends on neither.  Everything is queued
 * on the context's stream; one synchronisation at the end. */
int32_t cude_predictive_bands(cude_ctx* ctx, int32_t n_sets, const double* cond_sets, int32_t n_times, const double* times,
                              int32_t state, int32_t n_ranks, const int32_t* ranks, double* order_out, double* mean_out,
                              int32_t* bad_sets_out);

/* Simulation-based prediction discrepancies pd and their decorrelated, normalised form npde per subject (Brendel et al.
 * 2006, Comets et al. 2008: what Monolix, saemix and NONMEM report after a SAEM fit), reduced on the device: do the observed
 * data look like draws from the fitted (network, mu, Omega, sigma)?  The reference has no such diagnostic; the host loop this
 * replaces is n_sims x (cude_set_params, cude_simulate, a download of the trajectories) and numpy.  The host receives
 * per-subject rows, never the simulations (unless it asks for them).
 *   1. Rows: the R = T - 1 data times t_1 ... t_{T-1} of state `state`; t_0 is the initial state and is never drawn.
 *      C-peptide models: state must be 0, the observed state (the observation is the population's own row).  Suppression
 *      model: state 0, 1 or 2 (the observation is that state's data row).  R <= 31 (n_obs <= 32).
 *   2. Random effects: set k uses cond_sets[k] ([n_sims][N] row-major), or with cond_sets == NULL prior_mean + prior_sd z: the
 *      product rounded, then the sum (no fma); z a standard normal of the context's Philox key (cude_set_rng), counter =
 *      (global subject, first_rep + k) in a block kind no other entry point uses, Box-Muller as the Metropolis draws.
 *      2 <= n_sims <= 4096, 0 <= first_rep, first_rep + n_sims <= 2^47.
 *   3. Solve: set k is solved exactly as cude_predictive_bands rule 1 solves a set at the data's own times: v[k, r, i] has the
 *      bits of cude_simulate's state `state` at t_{r+1} after cude_set_params(ctx, NULL, cond_sets[k]).
 *   4. Simulated observation: y_sim[k, r, i] = v[k, r, i] + (sigma[i] s) eps[k, r, i], every operation rounded on its own; s =
 *      the state's cude_get_scale value (suppression) or 1 (c-peptide).  eps = noise[(k R + r) N + i] ([n_sims][R][N]), or
 *      with noise == NULL a Philox normal of a second block kind of its own with counter (global subject, first_rep + k,
 *      row r).  A draw depends on (seed, global subject, replicate, row) alone: not on the chunking, not on the sharding
 *      (cude_set_rng's subject_offset).  cude_npde_draws returns exactly the normals a call with NULL inputs uses:
 *      eta_normals_out [n_sims][N] (the z of rule 2), noise_out [n_sims][R][N]; either may be NULL, not both.
 *   5. Used simulations: a simulation with a non-finite y_sim in any row is left out for that subject; n_used_out[i] counts
 *      the rest.  sims_out (optional, [n_sims][R][N]) returns y_sim, left-out simulations included.
 *   6. Moments over the used simulations, in replicate order: m_r = (((y_0r + y_1r) + ...)) / n_used; C_rs = (sum_k
 *      (y_kr - m_r) (y_ks - m_s)) / (n_used - 1), the sum started at +0.0, each product rounded, then added (no fma).
 *      pred_mean_out, pred_var_out ([R][N]) = m and the diagonal of C.
 *   7. pd: below_out[r N + i] = #{k used : y_kr < y_obs_r}, strict and exact; pd_out = below / n_used clipped to
 *      [1 / (2 n_used), 1 - 1 / (2 n_used)].
 *   8. Decorrelation: C = L L' row by row, sequential sums without fma: for s < r, L_rs = ((C_rs - L_r0 L_s0) - ... -
 *      L_r,s-1 L_s,s-1) / L_ss; the pivot p = (C_rr - L_r0^2) - ... - L_r,r-1^2, L_rr = sqrt(p).  A pivot with
 *      !(p > 2^-40 C_rr) sets CUDE_NPDE_SINGULAR.  w = L^-1 (y - m) by forward substitution, w_r = (((y_r - m_r) - L_r0 w_0) -
 *      ... - L_r,r-1 w_r-1) / L_rr, for the observation and for every used simulation; below_decorr_out[r N + i] = #{k used
 *      : w_kr < w_obs_r}; npde_out = Phi^-1(below_decorr / n_used, clipped as pd) by Wichura's AS241 (PPND16), written out in
 *      the library.
 *   9. status_out[i], bits: CUDE_NPDE_SINGULAR (below_decorr = -1, npde = NaN; pd is still given); CUDE_NPDE_FEW (n_used <=
 *      R: treated as singular, the factorisation is not attempted); CUDE_NPDE_FAILED_SIMS (n_used < n_sims);
 *      CUDE_NPDE_BAD_OBS (a non-finite observation in a row, or a non-finite sigma[i]: every double output NaN, every
 *      count -1, n_used included).  cude_n_failed afterwards counts the subjects with SINGULAR, FEW or BAD_OBS.  Other
 *      subjects are unaffected, bit for bit.
 *  10. All n_sims simulations of a subject are resident when it is reduced: the solves are split over whole workgroups of 64
 *      subjects by ~1 GB of trajectories and simulated observations (option "npde_subjects" forces the split), and every
 *      output is bit-identical for every split and every sharding.
 *  11. CUDE_ERR_UNSUPPORTED for a network on the fallback kernel (cude_set_network), whose dense output takes one parameter
 *      set; CUDE_ERR_STATE under stream capture, without a population or shared parameters; CUDE_ERR_ARG for n_sims or
 *      first_rep out of range, a bad state, a null or negative sigma entry, prior_sd not > 0 (or a non-finite prior) while
 *      cond_sets == NULL, or no output requested.  Leaves the context's parameters and the position of its Metropolis stream
 *      untouched.  Adaptive mode: cude_adaptive_steps refuses afterwards.
 * All outputs optional, at least one.  One multi-set dense-output launch per pass, then the reduction; one stream, no
 * graph, one synchronisation per pass. */
#define CUDE_NPDE_SINGULAR    1
#define CUDE_NPDE_FEW         2
#define CUDE_NPDE_FAILED_SIMS 4
#define CUDE_NPDE_BAD_OBS     8
int32_t cude_npde(cude_ctx* ctx, int32_t n_sims, const double* cond_sets, double prior_mean, double prior_sd,
                  const double* sigma, int64_t first_rep, const double* noise, int32_t state, double* pred_mean_out,
                  double* pred_var_out, int32_t* below_out, int32_t* below_decorr_out, double* pd_out, double* npde_out,
                  int32_t* n_used_out, int32_t* status_out, double* sims_out);
int32_t cude_npde_draws(cude_ctx* ctx, int64_t first_rep, int32_t n_sims, double* eta_normals_out, double* noise_out);

/* Visual predictive check by subject group (what Monolix, saemix, NONMEM/PsN and nlmixr plot after a SAEM fit; the
 * reference stratifies what it plots by NGT / IGT / T2DM, `train_data.types`), reduced on the device: n_sims data sets are
 * simulated from the fitted (network, mu, Omega, sigma); inside each stratum of subjects the quantiles ACROSS SUBJECTS of
 * every simulated data set are taken at every data time, then an interval across the simulations of each such quantile,
 * next to the same quantiles of the observed data.  The host route this replaces is cude_npde(..., sims_out), a download
 * of [n_sims][R][N] doubles and numpy.quantile over subjects, then over simulations.
 *   1. Simulation: rows, random effects, solve and simulated observations are cude_npde's rules 1 ... 4 word for word: with
 *      the same context, seed, first_rep, cond_sets, noise, sigma and state, y_sim[k, r, i] has the bits of cude_npde's
 *      sims_out.  2 <= n_sims <= 4096, R = T - 1 <= 31.
 *   2. Groups: group[i] in [0, n_groups) is subject i's stratum (group == NULL: everybody in group 0), 1 <= n_groups <= 8.
 *      A negative id leaves the subject out of every stratum and sets CUDE_VPC_NO_GROUP (alone: such a subject is not
 *      looked at further); an id >= n_groups is CUDE_ERR_ARG.  A subject with a non-finite observation in any row, or a
 *      non-finite sigma[i], is left out of its group throughout and gets CUDE_VPC_BAD_OBS.  n_members_out[g] counts the
 *      subjects that remain: the members.
 *   3. Quantile of n values at level q (type 7: Julia's `quantile`, numpy.quantile's default): h = (n - 1) q in double,
 *      lo = floor(h), hi = min(lo + 1, n - 1), g = h - lo, d = x_hi - x_lo; the value is x_hi - d (1 - g) when g >= 1/2,
 *      otherwise x_lo + d g, every operation rounded on its own (no fma).  x_lo, x_hi are exact order statistics: values of
 *      the column, selected and not computed.  Where a column holds both -0.0 and +0.0 the sign of a selected zero is
 *      unspecified.  levels [n_levels] and ci_levels [n_ci] are strictly increasing inside [0, 1], 1 <= n_levels <= 8,
 *      1 <= n_ci <= 8.
 *   4. Observed quantiles: obs_q_out[(g R + r) L + l] = rule 3 at levels[l] over the observations of group g's members in
 *      row r (L = n_levels).
 *   5. Simulated quantiles: sim_q_out[((k G + g) R + r) L + l] = the same quantile of y_sim[k, r, .] over group g's members
 *      (G = n_groups).  A simulation in which any member of group g has a non-finite y_sim in any row is left out for that
 *      group: its sim_q entries are NaN in every row and level, and that member gets CUDE_VPC_FAILED_SIMS.
 *      n_sims_used_out[g] counts the simulations that remain (n_sims for a group without members: none is left out).  Other
 *      groups are unaffected, bit for bit.
 *   6. Interval across simulations: sim_ci_out[((g R + r) L + l) C + c] = rule 3 at ci_levels[c] over the n_sims_used[g] used
 *      values sim_q[., g, r, l] (C = n_ci).  A group with no member or no used simulation has NaN in all its double outputs.
 *   7. status_out[i]: the CUDE_VPC_* bits.  cude_n_failed afterwards counts the subjects with BAD_OBS or FAILED_SIMS.  All N
 *      subjects of a simulation are resident when it is reduced: the passes are split over simulations by ~1 GB of
 *      trajectories and simulated observations (option "vpc_sims" forces the simulations per pass), and every output is
 *      bit-identical for every split.
 *   8. CUDE_ERR_UNSUPPORTED for a network on the fallback kernel (cude_set_network), as cude_npde; CUDE_ERR_STATE under stream
 *      capture, without a population or shared parameters; CUDE_ERR_ARG for n_sims, first_rep, n_groups, n_levels or n_ci
 *      out of range, levels that do not increase strictly inside [0, 1], a group id >= n_groups, a bad state, a null or
 *      negative sigma entry, prior_sd not > 0 (or a non-finite prior) while cond_sets == NULL, or none of obs_q_out,
 *      sim_ci_out, sim_q_out requested.  Leaves the context's parameters and the position of its Metropolis stream
 *      untouched.  Adaptive mode: cude_adaptive_steps refuses afterwards.
 *   9. The quantiles are over the context's OWN subjects: no exchange is used, a sharded population gets shard-local strata
 *      (gather the shards' sims through cude_npde if population-wide strata are wanted).
 * All outputs optional, at least one of the first three.  Per pass one multi-set dense-output launch, the observations, and
 * per group one selection launch: columns of at most 4096 members on the shared sorting tile, longer ones through a radix
 * select that works from the column in device memory (option "vpc_select" = 1: every column; tests).  One stream, no graph,
 * one synchronisation per pass. */
#define CUDE_VPC_NO_GROUP    1
#define CUDE_VPC_FAILED_SIMS 2
#define CUDE_VPC_BAD_OBS     4
int32_t cude_vpc(cude_ctx* ctx, int32_t n_sims, const double* cond_sets, double prior_mean, double prior_sd,
                 const double* sigma, int64_t first_rep, const double* noise, int32_t state,
                 int32_t n_groups, const int32_t* group, int32_t n_levels, const double* levels,
                 int32_t n_ci, const double* ci_levels,
                 double* obs_q_out, double* sim_ci_out, double* sim_q_out,
                 int32_t* n_members_out, int32_t* n_sims_used_out, int32_t* status_out);

/* The per-set objective of per-subject values and its per-subject argmin -- `likelihood_values` / `map_objective_values`
 * over the kept samples and their `argmax` / `argmin`, from which the MLE / MAP LBFGS runs start
 * (c-peptide/06-saem.jl:226-235).  SSE_i(cond_sets[k][i]) for every set ([n_sets][N] row-major) through
 * cude_profile_conditional's launches, chunked like a profile scan (option "profile_chunk"): the SSE bits equal
 * cude_profile_conditional's wherever a set holds one value for everybody.  F = SSE + pw (x - pc)^2 rounded as
 * cude_profile_intervals rule 1; reduced on the device to best_objective_out[i] = min_k F and best_index_out[i] = its set
 * index (strict <: the first minimum wins; a non-finite F is above everything; no finite value: index 0, +Inf).
 * sse_out [n_sets][N], best_index_out [N], best_objective_out [N]: all optional, at least one.  Every model and both
 * modes, the fallback kernel included; CUDE_ERR_STATE under stream capture.  Leaves the context's parameters untouched;
 * adaptive mode: cude_adaptive_steps refuses afterwards. */
int32_t cude_evaluate_conditional_sets(cude_ctx* ctx, int32_t n_sets, const double* cond_sets, double penalty_weight,
                                       double penalty_center, double* sse_out, int32_t* best_index_out,
                                       double* best_objective_out);

/* Per-subject marginal log-likelihoods, the random effect integrated out on the device:
 *   log L_i = log of the integral over eta of exp(individual_log_likelihood(eta) + logpdf(Normal(prior_mean, prior_sd), eta))
 * (src/saem.jl:55-66; the exponent is minus `map_objective`, src/saem-symreg.jl:68-73), by a quadrature rule shared by all
 * subjects or by self-normalised importance sampling, together with the posterior moments that fall out of the same sums.
 * The sum of logml_out over the subjects is the population's marginal log-likelihood (AIC, BIC, likelihood-ratio tests).
 * The host receives a handful of numbers per subject, never the n_nodes x N SSEs.
 *   1. Points: x_ik = center_i + scale_i z_ik, the product rounded, then the sum (no fma contraction: numpy's
 *      center + scale * z has the same bits); center[N] NULL = the context's conditional parameters, scale[N] NULL = 1.
 *      Shared rule (nodes given): z_ik = nodes[k], a_ik = log_weights[k], both finite.  Device draws (nodes ==
 *      log_weights == NULL): z_ik = the standard normal of the context's Philox stream for (subject i, step first_step +
 *      k) -- the bits cude_rng_draws(ctx, first_step, n_nodes, normals, NULL) returns -- and a_ik = c_K + 0.5 (z z),
 *      c_K = 0.5 log(2 pi) - log(n_nodes) formed once on the host: self-normalised importance sampling from
 *      Normal(center_i, scale_i^2).  The context's own stream position (cude_set_rng, the Metropolis steps) is neither
 *      read nor advanced.
 *   2. Term: t_ik = (a_ik + ll_ik) + lp_ik.  ll_ik = fma(-SSE, 1/(2 sigma^2), -(T/2) log sigma^2), cude_mh_estep's
 *      log-likelihood at temperature 1 (the reference's convention: no 2 pi constant).  lp_ik = (-0.5 (u u) - log prior_sd)
 *      - 0.5 log(2 pi) with u = (x - prior_mean) / prior_sd, every operation rounded on its own; 0 when prior_sd = +Inf.
 *      SSE_i(x_ik) comes from cude_evaluate_conditional_sets's launches: its bits equal that function's sse_out at
 *      cond_sets = points_out.  A non-finite SSE is a bad node, t = -Inf; so is a node whose term is not finite for any
 *      other reason (an overflow).  A non-finite center_i, or a scale_i that is not finite and > 0, makes all nodes of
 *      subject i bad.
 *   3. Accumulation: one lane per subject, in node order k = 0 ... n_nodes - 1, state (M, S0, S1, S2, S3, Q) = (-Inf, 0, 0,
 *      0, 0, 0).  A bad node is skipped.  For t > M: r = exp(M - t); S0 ... S3 are multiplied by r and Q by r r; M = t and
 *      e = 1.  Otherwise e = exp(t - M).  Then S0 += e, S1 += e z, S2 += e (z z), S3 += e SSE, Q += e e (no fma).  The
 *      state lives in device memory between the chunks (option "profile_chunk" = nodes per launch), and a subject's nodes
 *      are folded in strictly in order: every output is bit-identical for every chunk size.
 *   4. Result: logml = (M + log S0) + log scale_i; post_mean = center + scale (S1/S0); post_var = scale^2 max(0, S2/S0 -
 *      (S1/S0)^2); post_sse = S3/S0 (the posterior expectation of the SSE: with post_mean and post_var it gives the exact EM
 *      updates of sigma^2, mu and Omega^2); ess = S0^2 / Q (Kish's effective sample size); n_bad = the number of bad nodes.
 *      A subject with no finite term gets logml = -Inf and NaN in the other four doubles; cude_n_failed counts these
 *      subjects afterwards.  Other subjects are unaffected, bit for bit.
 *   5. Both network models, the symbolic model in either cond_space, fixed-step and adaptive mode, the fallback kernel.
 *      A sharded population needs no exchange: every output is per subject.  1 <= n_nodes <= 65536.  CUDE_ERR_ARG: one of
 *      nodes / log_weights NULL but not the other, a non-finite node or weight, first_step < 0, sigma not finite and > 0,
 *      prior_sd not > 0 (or NaN), prior_mean not finite, no output requested.  CUDE_ERR_STATE: no population or shared
 *      parameters, center == NULL without conditional parameters, stream capture.  Leaves the context's parameters
 *      untouched.  Adaptive mode: cude_adaptive_steps refuses afterwards.  Everything is queued on the context's stream;
 *      one synchronisation at the end.
 * Outputs: logml_out, post_mean_out, post_var_out, post_sse_out, ess_out, n_bad_out [N]; points_out, terms_out
 * [n_nodes][N] row-major (x_ik and t_ik); all optional, at least one.
 * Limitation: a rule or a proposal centred at ONE mode misses mass elsewhere.  CPU-oracle measurements (N = 6, a 2-4-4-1
 * network, 30 steps, sigma ~ 0.027, prior Normal(-1, 0.8^2)), 33-node Gauss-Hermite at the MAP with the Laplace scale
 * against a 16 001-point trapezoid over mu +- 8 Omega: four subjects agreed to 1e-13 ... 1.5e-9, a wide skewed one to
 * 6.4e-9, and one subject with ~7 % of its posterior mass away from the mode came out 0.070 short at every rule size.
 * Laplace (one node): gaps of 4e-4 ... 0.07.  Trapezoid 16 001 against 8 001 points: 1e-14.  Importance sampling with 2048
 * draws: within its own standard errors, ess 1 300 ... 2 047.  A fixed grid (center 0, scale 1, trapezoid weights) is the
 * robust route. */
int32_t cude_marginal_likelihood(cude_ctx* ctx, int32_t n_nodes, const double* nodes, const double* log_weights,
                                 int64_t first_step, const double* center, const double* scale, double sigma,
                                 double prior_mean, double prior_sd, double* logml_out, double* post_mean_out,
                                 double* post_var_out, double* post_sse_out, double* ess_out, int32_t* n_bad_out,
                                 double* points_out, double* terms_out);

/* Per-subject scores with respect to the shared (network) parameters: the weighted gradient rows
 *   s_i = sum_k w_ik d SSE_i(x_ik) / d theta                                                              [P] per subject
 * that every other gradient call sums over the subjects before anyone sees them, their sum, and their cross product
 * sum_i s_i s_i^T (the outer-product-of-gradients information matrix; the "S matrix" of the pharmacometric tools).  With the
 * posterior weights of cude_marginal_likelihood's nodes, -sum_i s_i / (2 sigma^2) is the network gradient of the marginal
 * log-likelihood (Fisher's identity); with 0/1 or bootstrap weights it is a per-subject weighting of the shared gradient.
 *   1. Sets: set k is the context's shared parameters with the conditional vector cond_sets[k] ([n_sets][N] row-major);
 *      cond_sets NULL with n_sets == 1 = the context's conditional parameters.  A set is solved as
 *      cude_multistart_loss_grad solves one -- the fixed-step map, or the accepted steps of the adaptive solve taken as
 *      fixed arithmetic -- always on the one-lane kernels, and row_ik = d SSE_i(x_ik) / d theta is the lane's own gradient
 *      right before those kernels add the lanes up: no 1/N, no L2 term.
 *   2. Weights: weights [n_sets][N] row-major, finite; NULL = 1.  s_i = s_i + (w_ik row_ik) in set order k = 0 ... n_sets - 1
 *      from 0, the product rounded, then the sum (no fma contraction); wsse_i = sum_k w_ik SSE_i(x_ik) by the same rule.  A
 *      set with w_ik == 0 is skipped for subject i, whatever its solve gave: a bad quadrature node without posterior weight
 *      poisons nothing.  The state lives in device memory between the launches (sets per launch: the scratch budget, and
 *      option "profile_chunk"), and a subject's sets are folded in strictly in order by one lane: every output is
 *      bit-identical for every chunking.
 *   3. Failed subjects: a set with w_ik != 0 whose SSE or row is not finite makes subject i failed (so does a weighted sum
 *      that overflows).  bad_out[i] counts such sets.  A failed subject gets NaN in its score row and wsse, is left out of
 *      sum and cross, and is counted by cude_n_failed afterwards.  Other subjects are unaffected, bit for bit.
 *   4. Parameter mask (cude_set_param_mask): every row is multiplied by it; a masked entry is exactly 0.0 in score_out (a
 *      failed subject's row included), sum_out and cross_out.
 *   5. Sum and cross product over the subjects that did not fail: sum[q] = sum_i s_i[q], cross[q][r] = sum_i s_i[q] s_i[r].
 *      Both triangles of cross are written and equal bit for bit.  The order of the additions is fixed by N alone (blocks of
 *      1024 subjects in index order, the blocks in order) and the same from run to run.  They are formed on the device from
 *      the table there: the host never needs score_out to get them.  Sharded population: they are this rank's sums; the
 *      caller adds the ranks up (cude_comm_allreduce_host).
 *   6. Both network models, the symbolic model (P = 1) in either cond_space, fixed-step and adaptive mode, every tuned
 *      shape with any of its activation functions, and the fallback kernel.
 *   7. Leaves the context's parameters untouched.  Adaptive mode: cude_adaptive_steps refuses afterwards; a population of
 *      8192 subjects or more may be regrouped as by any multi-set gradient call (cude_adaptive_regroup), on which no
 *      per-subject result depends.
 *   8. CUDE_ERR_ARG: n_sets < 1, cond_sets == NULL with n_sets > 1, a non-finite weight, no output requested.
 *      CUDE_ERR_STATE: no population or shared parameters, cond_sets == NULL without conditional parameters, stream capture.
 *   9. Everything is queued on the context's stream; one synchronisation at the end.
 * Outputs: score_out [N][P] row-major, wsse_out [N], bad_out [N], sum_out [P], cross_out [P][P]; all optional, at least one.
 * Not built: the terms of cude_marginal_likelihood are not handed over on the device (the caller forms the n_sets x N
 * weights from terms_out and passes them back in), and the forward half of every set's solve runs again under the adjoint. */
int32_t cude_subject_scores(cude_ctx* ctx, int32_t n_sets, const double* cond_sets, const double* weights,
                            double* score_out, double* wsse_out, int32_t* bad_out, double* sum_out, double* cross_out);

/* Output Jacobians with respect to the shared (network) parameters and the expected-information (Gauss-Newton) matrices of
 * a least-squares fit built from them.  With J_io = d yhat_io / d theta [P] and jc_io = d yhat_io / d cond_i for subject i and
 * output o, and the loss's own weights w_o:
 *   A   = sum_i sum_o w_o J_io^T J_io            [P][P]  information for theta with the conditionals taken as known
 *   b_i = sum_o w_o jc_io J_io                   [P]     coupling of theta with subject i's own conditional parameter
 *   d_i = sum_o w_o jc_io^2                              (cude_sensitivity's info)
 *   S   = A - sum_i b_i b_i^T / (d_i + pw)       [P][P]  Schur complement of the arrowhead matrix [[A, B], [B^T, D + pw I]]:
 *                                                        the information for theta with the conditionals fitted
 *   qform_io = z C z^T, z = J_io - (profiled ? jc_io / (d_i + pw) : 0) b_i: with C = pinv(S) and profiled = 1,
 *              qform_io + jc_io^2 / (d_i + pw) is the delta-method variance of yhat_io in units of sigma^2.
 * The rank of A is bounded by N (n_out - 1), not by N as the rank of cude_subject_scores' cross product is.
 *   1. Outputs: c-peptide models (n_state 2 or 3) n_out = T, o = j: state 1 at the data's time j, w_o = 1.  Suppression
 *      model n_out = 3 T, o = s + 3 j (the order of cude_forward's traj), w_o = 1 / scale_s^2.  cude_n_outputs reports n_out.
 *      The rows of the column t_0, and every row of suppression state 0, depend on no parameter: exactly +0.0, and no launch
 *      is spent on them.
 *   2. Rows: the live outputs are the sets of multi-set gradient launches on the one-lane kernels (as cude_subject_scores
 *      rule 1), whose reverse sweep is seeded with exactly 1.0 at that output and exactly 0.0 elsewhere instead of the
 *      residuals: the lane's row is J_io and its conditional gradient jc_io, in the state's own units (no 2, no 1/N, no
 *      1/scale^2).  Adaptive mode: the derivative of the accepted-step map, the adjoint's convention.  cond [N] = the
 *      conditional vector of every launch, replicated on the device; NULL = the context's.
 *   3. Launch shape: live outputs per launch by the scratch budget and option "profile_chunk".  b_i and d_i are folded by one
 *      lane per (subject, parameter) in output order o = 0 ... n_out - 1 from 0, s = s + ((w_o jc_io) J_io) with every
 *      product and the sum rounded on their own (no fma contraction), in state that lives in device memory between the
 *      launches: every output of the call is bit-identical for every chunking.
 *      Cost: with ONE chunk the launches run once.  With several, qform_out needs b_i and d_i complete before the rows are
 *      read again, so the launches run a second time; without qform_out, A is summed along the first pass, the call
 *      synchronises once in between to learn whether a subject failed, and only then runs the launches again for A.
 *   4. A and S are summed over the subjects that did not fail with plain FMAs in an order fixed by (N, n_out) alone: blocks of
 *      1024 subjects; inside a block the outputs in order, inside an output the subjects in index order, acc = fma(w_o J_q,
 *      J_r, acc); then the blocks in block order.  Both triangles are written and equal bit for bit.  The Schur term is the
 *      same sum over t_i = b_i / sqrt(d_i + pw), and S = A - that, entry by entry.
 *   5. FLAT (status bit 2): a subject whose d_i + pw is not > 0.  Its Schur term is skipped, its qform uses z = J_io, and it
 *      is not a failure.
 *   6. FAILED (status bit 1): a subject with a non-finite row entry, jc or SSE of the solve at any live output (or a b_i / d_i
 *      that overflowed).  Every entry of its jac and jcond rows (masked columns: 0), coupling, dcond and qform is NaN; it is
 *      left out of A and S and counted by cude_n_failed afterwards.  Other subjects are unaffected, bit for bit.
 *   7. Parameter mask (cude_set_param_mask): every row is multiplied by it; a masked entry is exactly +0.0 in jac_out,
 *      coupling_out, and the rows and columns of gn_out and schur_out.
 *   8. Both network models, the symbolic model (P = 1) in either cond_space, fixed-step and adaptive mode, every tuned shape
 *      with any of its activation functions, and the fallback kernel.  Adaptive mode: cude_adaptive_steps refuses afterwards;
 *      a population of 8192 subjects or more may be regrouped as by cude_subject_scores (rule 7 there).
 *   9. Sharded population: A and S are this rank's sums (with this rank's Schur terms); they are additive over the ranks.
 *  10. CUDE_ERR_ARG: no output requested, qform_out without cov, a non-finite cov entry, penalty_weight negative or not
 *      finite.  CUDE_ERR_STATE: no population or shared parameters, cond == NULL without conditional parameters, stream
 *      capture.
 *  11. Leaves the context's parameters untouched.  Everything is queued on the context's stream; one synchronisation at the
 *      end (and the one of rule 3).  jac_out is written chunk by chunk.
 * Outputs (all optional, at least one): jac_out [N][n_out][P], jcond_out [N][n_out], gn_out [P][P], coupling_out [N][P],
 * dcond_out [N], schur_out [P][P], qform_out [N][n_out] (needs cov [P][P], finite), status_out [N].
 * A trainer on these matrices: cude_train_lm below.  Not built: sharing one forward solve among the outputs of a subject (every output's launch
 * row repeats it); an MFMA cross product; rows from the time-split and five-wave kernels; output times other than the
 * data's. */
#define CUDE_INFO_FAILED 1
#define CUDE_INFO_FLAT 2
int32_t cude_network_information(cude_ctx* ctx, const double* cond, double penalty_weight, const double* cov, int32_t profiled,
                                 double* jac_out, double* jcond_out, double* gn_out, double* coupling_out, double* dcond_out,
                                 double* schur_out, double* qform_out, int32_t* status_out);
/* Outputs per subject of cude_network_information (rule 1).  CUDE_ERR_STATE: no population. */
int32_t cude_n_outputs(cude_ctx* ctx, int32_t* n_out);

/* Levenberg-Marquardt on the matrices of cude_network_information, for the joint fit of the shared parameters theta [P]
 * and every subject's conditional parameter c_i.  With F = N loss = sum_i sum_o w_o r_io^2 + N lambda |theta|^2, the
 * half-gradients ghat_theta = sum w_o r_io J_io + N lambda theta and ghat_c,i = sum_o w_o r_io jc_io (N / 2 times what
 * cude_loss_grad returns) and the Gauss-Newton matrix H = [[A + N lambda I, B], [B^T, D]] (B's column i = b_i, D = diag d_i;
 * penalty weight 0), a step for the damping mu solves (H + mu M) [dtheta; dc] = -[ghat_theta; ghat_c].
 *   1. Scaling: M is diagonal, M_theta,q = max(A_qq + N lambda, 1e-8 max_r (A_rr + N lambda)), M_c,i = max(d_i, 1e-8 max_j
 *      d_j), and 1 wherever that maximum is not > 0.  A FLAT subject (d_i = 0) so gets a damped gradient step.
 *   2. The solve is by elimination, never as a dense (P + N) system: e_i = d_i + mu M_c,i; S_mu = A + N lambda I + mu
 *      diag(M_theta) - sum_i b_i b_i^T / e_i; rhs = -(ghat_theta - sum_i b_i ghat_c,i / e_i); S_mu dtheta = rhs by Cholesky;
 *      dc_i = -(ghat_c,i + b_i . dtheta) / e_i.  Predicted reduction pred = -ghat^T delta + mu delta^T M delta (in units of F;
 *      > 0 for a valid step).
 *   3. Order of the sums: sum_i b_i b_i^T / e_i is cude_network_information's cross product (rule 4 there: blocks of 1024
 *      subjects in index order) over t_i = b_i / sqrt(e_i); the right-hand sides and pred add 256 strided partial sums by a
 *      halving tree.  Everything is fixed by (N, P) alone: results are bit-identical from run to run.
 *   4. Cholesky: one workgroup per damping, S_mu in LDS for P <= 86 and in device memory above, up to P = 193 (the largest
 *      tuned shape; more: CUDE_ERR_UNSUPPORTED).  A pivot that is not > 0 or not finite, a non-finite step, or a FAILED
 *      subject of the information pass makes that candidate invalid: pred = loss = NaN (and NaN sets from
 *      cude_lm_candidates); other candidates are not touched.
 *   5. Parameter mask (cude_set_param_mask): the row and column of a masked entry of S_mu are the unit diagonal, its
 *      dtheta_q is exactly 0.0 and its value is copied, so that it keeps its bits.
 *   6. Trial losses: the candidates theta + dtheta_k, c + dc^k are written on the device as the sets of ONE multi-set forward
 *      launch; a loss is cude_multistart_forward's at that set, bit for bit (+Inf for a failed solve).
 *   7. Both network models, the symbolic model (P = 1), fixed-step and adaptive mode, every tuned shape and the fallback
 *      kernel, as cude_network_information (rule 8 there).
 *   8. CUDE_ERR_STATE: no population or parameters, stream capture.  CUDE_ERR_UNSUPPORTED: a sharded population (a
 *      communicator or the exchange), P > 193.  CUDE_ERR_ARG: a damping that is not finite and > 0, n_mu / n_trials outside
 *      1 ... 8, a negative tolerance, max_iters < 0, no output requested.
 *
 * cude_lm_candidates: the steps for the caller's dampings mu[n_mu] at the context's current parameters and their trial
 * losses; changes nothing in the context's parameters.  Outputs (all optional, at least one): nn_out [n_mu][P], cond_out
 * [n_mu][N], pred_out [n_mu], loss_out [n_mu], and the steps themselves dnn_out [n_mu][P], dcond_out [n_mu][N] (theta + dtheta
 * rounds, so a small step cannot be recovered from nn_out).
 *
 * cude_train_lm: the loop, on the context's parameters (as cude_adam_run leaves its result there).
 *   9. An iteration is one gradient launch, one information pass, and the K = n_trials dampings mu_k = mu 5^(k - 1),
 *      k = 0 ... K - 1 (clamped to [1e-15, 1e15]), solved and evaluated side by side.
 *  10. Selection, on the device by one lane: the candidate with the lowest finite trial loss below the current loss, ties to
 *      the lower index.  It is copied into the context's parameters and confirmed by the evaluation cude_forward makes there:
 *      accepted if that loss is finite and below the current one; then it is the current loss, and mu <- mu_k / 5, clamped
 *      to [1e-15, 1e15].  (The trial launch and cude_forward may take different kernels, whose sums differ in the last
 *      bits: the trace is cude_forward's value throughout, so that it strictly decreases over accepted iterations and
 *      cude_forward afterwards returns its last entry bit for bit.)  Otherwise the parameters are restored bit for bit and
 *      mu <- 25 mu_{K-1}: the next ladder continues this one upwards without a gap.  (The ratio was 3 at first: with
 *      four rungs a quarter of the iterations of a 12-subject fit were then rejected outright, because the damping that
 *      works moves by more than 3 between iterations; 5 lost fewer and ended lower from every start tried, 10 did not.)
 *  11. status: CUDE_LM_GRAD the max-norm of the loss gradient (cude_loss_grad's g_nn and g_cond) at the current point is
 *      <= gtol (checked before an iteration counts; the parameters are that point); CUDE_LM_DECREASE an accepted
 *      iteration with old - new <= ftol old; CUDE_LM_STALLED 25 mu_{K-1} left the clamp; CUDE_LM_MAX_ITERS; CUDE_LM_FAILED a
 *      non-finite loss, a failed subject of the gradient launch or a FAILED subject of the information pass at the current
 *      point (cude_n_failed counts them): the parameters stay as at the last accepted point.
 *  12. loss_trace [max_iters + 1] and mu_trace [max_iters + 1] (optional): entry 0 the start, entry t the loss and the
 *      damping after iteration t, for t <= *n_iters_out; later entries are not written.
 *  13. Per iteration the host reads five doubles of the device's record, the confirming loss pair and the information
 *      pass's failure count; never a vector of N entries or a P x P matrix.
 * Not built: a sharded population; several restarts in one call; box bounds on the conditionals. */
#define CUDE_LM_GRAD 0
#define CUDE_LM_DECREASE 1
#define CUDE_LM_STALLED 2
#define CUDE_LM_MAX_ITERS 3
#define CUDE_LM_FAILED 4
int32_t cude_lm_candidates(cude_ctx* ctx, int32_t n_mu, const double* mu, double* nn_out, double* cond_out, double* pred_out,
                           double* loss_out, double* dnn_out, double* dcond_out);
int32_t cude_train_lm(cude_ctx* ctx, int32_t max_iters, int32_t n_trials, double mu0, double gtol, double ftol,
                      double* loss_trace, double* mu_trace, int32_t* n_iters_out, int32_t* status_out);

/* SAEM E-step on the device: n_mc Metropolis-Hastings steps of every subject's conditional parameter
 * (`mcmc_step` src/saem.jl:86-108, applied n_mcmc_steps times with the stochastic-approximation update of the
 * chain state :177-186).  The chain state is the context's conditional parameters (updated in place); the
 * network is the context's current one.  normals / uniforms are the host's randn() / rand() draws, [n_mc][N]
 * row-major.  log-likelihood = -(T/2) log sigma^2 - SSE/(2 sigma^2) (:55-66), -Inf on a failed solve; prior
 * Normal(prior_mean, prior_sd); accept iff log u < prior ratio + (ll_new - ll_cur)/temperature; state <-
 * (1-gamma) state + gamma (accepted ? proposal : state).  The reference re-evaluates the current state's likelihood
 * at every step (:96-97); here that happens only for gamma != 1 (the state is then a blend that was never solved
 * at).  For gamma == 1 -- its burn-in phase and the posterior sampling loop -- the next state is exactly the
 * accepted proposal or the unchanged state and the solve is deterministic, so the known SSE is carried over: same
 * bits, n_mc + 1 ensemble solves instead of 2 n_mc.  accepted[N] (optional) receives per-subject acceptance
 * counts.  All launches are queued on the stream; the call synchronises once at the end.
 * normals == uniforms == NULL: the draws are generated on the device (cude_set_rng) -- nothing crosses PCIe. */
int32_t cude_mh_estep(cude_ctx* ctx, int32_t n_mc, const double* normals, const double* uniforms, double sigma,
                      double prior_mean, double prior_sd, double proposal_std, double temperature, double gamma,
                      int64_t* accepted);

/* The same chain with every state kept: samples[n_mc][N] (row-major) receives each subject's conditional parameter
 * after every step -- the per-individual posterior sampling loop that follows SAEM (`for _ in 1:3000; p_individual,
 * accepted = mcmc_step(...); push!(individual_samples, p_individual)`, c-peptide/06-saem.jl:107-112) for all
 * individuals at once.  samples may be NULL (then identical to cude_mh_estep). */
int32_t cude_mh_chain(cude_ctx* ctx, int32_t n_mc, const double* normals, const double* uniforms, double sigma,
                      double prior_mean, double prior_sd, double proposal_std, double temperature, double gamma,
                      int64_t* accepted, double* samples);

/* Freeze shared parameters: every network-gradient entry the library forms -- cude_loss_grad, the Adam updates, the
 * restarts of cude_train_restarts / cude_multistart_loss_grad, the partial rows of cude_loss_grad_partial -- is
 * multiplied by mask[q] (0 = frozen, 1 = free; mask[P], or NULL to lift it).  Frozen entries keep exactly the value
 * cude_set_params gave them under Adam and L-BFGS.  Use: `chain([w1, w2, ...], tanh)` with unequal widths
 * (src/neural-network.jl:42-58) is the equal-width network of width max(w) whose extra units have zero weights; frozen at
 * zero they stay that network (the host mirror's chain(widths) does exactly this). */
int32_t cude_set_param_mask(cude_ctx* ctx, const double* mask);

/* Device-side random draws for cude_mh_estep / cude_mh_chain (the `randn()` / `rand()` of mcmc_step, src/saem.jl:88,103)
 * when the caller passes no draw arrays: counter-based Philox4x32-10, key = seed, counter = (global subject index,
 * index of the Metropolis step since this call, kind); standard normals by Box-Muller on two 53-bit uniforms, uniforms
 * from 53 bits, both strictly inside (0, 1).  A draw depends only on (seed, subject_offset + local index, step): the
 * chain of a subject is the same whatever the launch shape and however the population is sharded (subject_offset =
 * global index of this context's first subject).  Successive calls continue the stream; this call rewinds it.
 * Default: seed 0x243F6A8885A308D3, offset 0. */
int32_t cude_set_rng(cude_ctx* ctx, uint64_t seed, int64_t subject_offset);

/* The draws steps first_step ... first_step + n_steps - 1 of that stream use, [n_steps][N] row-major each (either
 * pointer may be NULL): lets a caller replay a device-generated chain elsewhere (the parity tests feed them to the
 * oracle chain and to the host-supplied-draws path). */
int32_t cude_rng_draws(cude_ctx* ctx, int64_t first_step, int32_t n_steps, double* normals, double* uniforms);

/* Loss and gradient: replaces ForwardDiff.gradient(loss, theta) under AutoForwardDiff()
 * (parameter-estimation.jl:370; suppression_model.jl:155; saem.jl:120) by a discrete adjoint
 * of the same fixed-step map.  g_nn[P]; g_cond[N] may be NULL (stays on the device). */
int32_t cude_loss_grad(cude_ctx* ctx, double* loss, double* g_nn, double* g_cond);
int32_t cude_n_failed(cude_ctx* ctx, int64_t* n_failed);

/* Optimisers.Adam(eta) state (parameter-estimation.jl:176; suppression_model.jl:164; saem.jl:128).
 * Resets the moments and the step counter. */
int32_t cude_adam_init(cude_ctx* ctx, double lr, double beta1, double beta2, double eps);
/* One fused optimiser iteration on device-resident parameters: loss + gradient + (all-reduce of
 * [g_nn; sum loss; n_failed] when a communicator is attached) + Adam update of nn (replicated)
 * and cond (sharded).  loss may be NULL: then nothing is copied back and the call does not
 * synchronise (use cude_synchronize). The reported loss is the one BEFORE the update. */
int32_t cude_adam_step(cude_ctx* ctx, double* loss);
int32_t cude_synchronize(cude_ctx* ctx);
/* Diagnostic: resident waves per compute unit (4 SIMDs) the one-lane gradient kernel of this context gets from the
 * runtime (hipOccupancyMaxActiveBlocksPerMultiprocessor with the launch's LDS size) -- registers and LDS as compiled. */
int32_t cude_grad_occupancy(cude_ctx* ctx, int32_t* waves_per_cu);
/* n_iters optimiser iterations in one call (the `maxiters` loop of Optimization.solve(prob, Adam, maxiters),
 * src/parameter-estimation.jl:176): iterations are captured into hipGraphs (eight per graph, single ones for the
 * remainder) and replayed without host round trips; losses[n_iters] (optional) receives the loss BEFORE each update,
 * read back once at the end.  The peer-write exchange (cude_xchg_*) is part of the captured reduction kernels; with an
 * RCCL communicator as the transport the iterations are queued as plain launches (RCCL calls are not captured).
 * Adaptive populations of >= 8192 subjects are re-ordered by accepted-step count on a schedule that counts this entry
 * point's iterations (see cude_adaptive_regroup). */
int32_t cude_adam_run(cude_ctx* ctx, int32_t n_iters, double* losses);

/* --- bring-your-own collective (MPI.jl, gloo, ...) instead of the built-in RCCL path.
 * cude_loss_grad_partial returns this rank's un-reduced [g_nn(P); sum_i sse_i; n_failed] (gradient entries
 * already carry the 1/N_global factor, the L2 term is NOT included); the host sums the vectors of all
 * ranks and hands the result to cude_adam_apply, which adds the L2 term, forms the loss and runs the Adam
 * update.  cude_set_global_subjects tells the context the global subject count (and, for the suppression
 * model, the globally averaged `scale`, suppression_model.jl:126) when no communicator is attached. */
int32_t cude_set_global_subjects(cude_ctx* ctx, double n_global, const double* scale3 /* or NULL */);
int32_t cude_get_scale(cude_ctx* ctx, double* scale3, double* n_global);
int32_t cude_loss_grad_partial(cude_ctx* ctx, double* partial /* P+2 */, double* g_cond /* N or NULL */);
int32_t cude_adam_apply(cude_ctx* ctx, const double* reduced /* P+2 */, double* loss);
/* The same exchange WITHOUT the host round trip, for a collective that reduces device memory in place (RCCL through
 * another binding, GPU-aware MPI): cude_partial_buffer hands out the device address of the context's P+2 doubles,
 * cude_loss_grad_partial_device fills them with this rank's un-reduced vector and synchronises the context's stream,
 * the caller all-reduces them in place on a stream of its own and waits for that, cude_adam_apply_device continues as
 * cude_adam_apply does.  (No reference line: the reference has no collective; this is the sharded form of
 * ForwardDiff.gradient + Optimisers.update, src/parameter-estimation.jl:170-176.) */
int32_t cude_partial_buffer(cude_ctx* ctx, double** device_ptr, int32_t* count /* P+2 */);
int32_t cude_loss_grad_partial_device(cude_ctx* ctx);
int32_t cude_adam_apply_device(cude_ctx* ctx, double* loss);

/* Average device time (ms) of the ensemble launches (forward, or forward+adjoint: whatever the calls since the last
 * query ran) measured with HIP events on the context's stream; resets the accumulator. */
int32_t cude_kernel_time_ms(cude_ctx* ctx, double* avg_ms, int64_t* launches);
/* The same samples with their median and minimum (the median is the sturdier figure when a few launches of the timed
 * region ran before the GPU clock had settled); resets the accumulator as cude_kernel_time_ms does. */
int32_t cude_kernel_time_stats(cude_ctx* ctx, double* avg_ms, double* median_ms, double* min_ms, int64_t* launches);
/* Enable / disable (0) the event timing used by cude_kernel_time_ms: 1 = a pair of HIP events around every ensemble
 * launch, n > 1 = around every n-th launch (a pair costs ~4.5 us of stream time and keeps queued iterations from being
 * replayed as graphs: sampling keeps a live kernel time at a fraction of that). */
int32_t cude_set_kernel_timing(cude_ctx* ctx, int32_t enabled);

/* --- multi-GPU: subjects are sharded, one context (process) per GPU; the only exchange is one
 * sum all-reduce of P+2 doubles per optimiser step (the reference has no distributed path; this
 * is the data-parallel form of EnsembleThreads, suppression_model.jl:113,123).
 * rank 0 creates the id, the host distributes its bytes, every rank calls cude_comm_init.
 * Multi-process RCCL on hosts without legacy IPC needs HSA_ENABLE_IPC_MODE_LEGACY=0 in the environment before the
 * process first touches the GPU; cude_comm_init with n_ranks > 1 returns CUDE_ERR_COMM if it is not set. */
int32_t cude_comm_unique_id(uint8_t id[CUDE_UNIQUE_ID_BYTES]);
int32_t cude_comm_init(cude_ctx* ctx, int32_t n_ranks, int32_t rank, const uint8_t id[CUDE_UNIQUE_ID_BYTES]);
/* Sum all-reduce of a host vector through the communicator (used for population statistics
 * such as SAEM's mean/var of the random effects, saem.jl:204-205). */
int32_t cude_comm_allreduce_host(cude_ctx* ctx, double* values, int32_t count);
/* What the attached communicator itself reports: ncclCommCount, ncclCommUserRank, ncclGetVersion (1, 0, 0 without a
 * communicator) -- lets a launcher prove which transport and how many ranks a multi-GPU run really used. */
int32_t cude_comm_info(cude_ctx* ctx, int32_t* n_ranks, int32_t* rank, int32_t* version);

/* --- multi-GPU without a collective library: the peer-write exchange.  Same role as the communicator above (the
 * data-parallel form of EnsembleThreads, suppression_model.jl:113,123; the one sum of P+2 doubles per optimiser step
 * that replaces ForwardDiff's accumulation over all subjects, src/parameter-estimation.jl:126-140,370), built for this
 * message size: every rank owns a mailbox in its GPU's memory, mapped into its peers through HIP IPC; the kernel that
 * finishes a rank's [g_nn; sum loss; n_failed] writes each double straight into a slot of EVERY rank's mailbox over
 * xGMI (two 8-byte words carrying the step's sequence number: a word is valid when its sequence matches, so no fence
 * and no flag ordering is needed), waits for the other ranks' words in its own mailbox and adds the n_ranks values IN
 * RANK ORDER.  Every rank therefore forms bit-identical sums, run to run and whatever the arrival order; there is no
 * extra launch in the step, and cude_adam_run keeps replaying captured graphs (it cannot with RCCL calls).  A wait
 * that sees no peer for `timeout_s` gives up: the step's loss becomes NaN and the next call that synchronises returns
 * CUDE_ERR_COMM (a kernel never spins for ever).
 *   every rank:  cude_xchg_export(ctx, n_ranks, rank, mine)        -> 128 bytes describing its mailbox
 *   the host:    all-gather of those bytes (any channel: torch.distributed, MPI.jl, a file)
 *   every rank:  cude_xchg_attach(ctx, all[n_ranks][128], timeout_s)   (collective: ends with a self-test)
 *   the host:    do ALL ranks report CUDE_OK?  (one logical AND over the ranks, same channel)
 *                no -> every rank, the successful ones too: cude_xchg_detach(ctx), and from the top: the next export
 *                      offers the next kind of mailbox memory (uncached device memory, then fine-grained, then ordinary
 *                      device memory -- the last only when all ranks share one device, or with option
 *                      "xchg_allow_plain"); after the third kind cude_xchg_export fails and the caller falls back to
 *                      cude_comm_init (RCCL).  cude/parallel.py `attach_exchange` and julia/CUDEHip.jl `attach_exchange!`
 *                      are this loop.
 * A kind is given up by the exporting rank itself when its allocation, clearing or hipIpcGetMemHandle fails; by all
 * ranks when any rank cannot open a peer's handle or fails the self-test (4 sum rounds over every column and both
 * parities with values that change per round, one max round) -- whether a peer ON ANOTHER DEVICE can write a given
 * kind is only known then.  A rank whose export failed contributes 128 zero bytes, which fails everybody's attach.
 * Ranks may live in one process (several contexts; at most 4 per device: their spinning reduction kernels share the
 * device's hardware queues -- a rehearsal configuration) or in several; all on ONE node.  Attach before the population is
 * uploaded, as with cude_comm_init (the global subject count is summed there).  With an exchange attached every
 * reduction of the library goes through it and no RCCL communicator is needed; when both are attached the exchange
 * is used while enabled (cude_xchg_enable(ctx, 0) switches to the communicator, for comparisons).  Every entry point
 * that synchronises behind an exchange launch reads the exchange's status word (page-locked host memory) and returns
 * CUDE_ERR_COMM if a wait gave up in ANY column. */
int32_t cude_xchg_export(cude_ctx* ctx, int32_t n_ranks, int32_t rank, uint8_t handle[CUDE_XCHG_HANDLE_BYTES]);
int32_t cude_xchg_attach(cude_ctx* ctx, const uint8_t* handles /* [n_ranks][CUDE_XCHG_HANDLE_BYTES] */, double timeout_s);
/* Releases this context's exported or attached exchange (no-op when a failed cude_xchg_attach already has); the next
 * cude_xchg_export starts one kind further down the order of preference than the last one did (the ranks move through
 * these levels together). */
int32_t cude_xchg_detach(cude_ctx* ctx);
int32_t cude_xchg_enable(cude_ctx* ctx, int32_t enabled);
/* n_ranks / rank of the attached exchange (1, 0 without), how its mailbox memory was allocated (3 = uncached, 1 =
 * fine-grained, 0 = ordinary device memory) and how many device-side waits have run out of time so far. */
int32_t cude_xchg_info(cude_ctx* ctx, int32_t* n_ranks, int32_t* rank, int32_t* memory_kind, int32_t* timeouts);

/* --- run-time options.
 * The network's activation functions -- `chain(widths, activations; output_activation)`, src/neural-network.jl:42-58 --:
 * "hidden_activation" = "tanh" (default) | "relu" | "sigmoid", "output_activation" = "softplus" (default) | "identity";
 * set them before the population is uploaded.  tanh / softplus (every network of the reference's scripts) run on the
 * tuned kernels; the other combinations on the general evaluation path of the same kernels, compiled for the shapes
 * 2-4-4-1, 2-6-6-1, 3-4-4-1 (c-peptide) and 4-3x5-1, 4-3x3-1 (suppression): CUDE_ERR_UNSUPPORTED otherwise.
 * Implementation switches (cude_ctx.h `Options` lists them): launch-path override of the tests ("cpep_path" = "1" |
 * "2:L" | "3:B:L"), "cpep_keep", "supp_store", "supp_ckpt", "tape_steps", "exp_table", "ms_split", "auto_regroup",
 * "poll_pinned", "debug_selector", "xchg_allow_plain", "xchg_fail_kinds" (tests), "force_fallback" (tests: cude_set_network takes the fallback kernel for tuned shapes too), "adaptive_team" (adaptive mode, small c-peptide
 * populations: a step's five network evaluations on five waves; 0 = the one-wave kernels), "fit_spec" (cude_fit_conditional: probes per forward launch, 0 = one, 1 ... 4 = golden-section steps per launch, -1 = by size), "mh_spec" (speculative Metropolis steps per
 * launch pair in cude_mh_estep / cude_mh_chain: 0 off, 2 ... 4, -1 = by population size; the chain is the same bit for bit),
 * "dense_chunk" (cude_simulate: output times per launch, 0 = ~1 GB of scratch; tests force several launches with it),
 * "dense_layout" (cude_simulate, suppression model: 0 = the caller's layout written directly, the default; 1 =
 * lane-contiguous rows + a transpose kernel), "refine_fused" (cude_refine_conditional in fixed-step mode: 1 = the one-launch
 * kernel, the default; 0 = one tangent launch per evaluation), "profile_chunk" (cude_profile_conditional / cude_profile_intervals:
 * grid points per launch, 0 = ~512 MB of scratch; tests force several launches with it), "predictive_subjects" /
 * "predictive_times" (cude_predictive_bands: subjects per solve launch, rounded up to 64, and output times per launch; 0 =
 * by the ~1 GB budget of sample trajectories; tests force several launches in either dimension with them), "bootstrap_chunk" /
 * "bootstrap_subjects" (cude_bootstrap_conditional: replicates per launch and subjects per pass, rounded up to 64; 0 = by the
 * ~256 MB / ~1 GB budgets; tests force either split with them), "npde_subjects" (cude_npde: subjects per pass, rounded up to 64; 0 =
 * by the ~1 GB budget; tests force the split with it), "vpc_sims" (cude_vpc: simulations per pass; 0 = by the ~1 GB budget;
 * tests force the split with it), "vpc_select" (tests: 1 = every column of cude_vpc's reduction over subjects goes through
 * the radix select).  Values are decimal integers as text unless noted.  Every option is also read once
 * at cude_create from its environment variable (CUDE_CPEP_PATH, CUDE_CPEP_KEEP, CUDE_SUPP_STORE, CUDE_SUPP_CKPT,
 * CUDE_TAPE_STEPS, CUDE_NO_EXPTAB, CUDE_NO_MS_SPLIT, CUDE_NO_AUTO_REGROUP, CUDE_NO_POLL_PINNED, CUDE_DEBUG_SELECTOR, CUDE_ALLOW_PLAIN_MAILBOX, CUDE_XCHG_FAIL_KINDS, CUDE_MH_SPEC, CUDE_FIT_SPEC, CUDE_NO_ADAPTIVE_TEAM, CUDE_DENSE_CHUNK, CUDE_DENSE_LAYOUT, CUDE_REFINE_FUSED, CUDE_PROFILE_CHUNK,
 * CUDE_PREDICTIVE_SUBJECTS, CUDE_PREDICTIVE_TIMES, CUDE_BOOTSTRAP_CHUNK, CUDE_BOOTSTRAP_SUBJECTS, CUDE_NPDE_SUBJECTS, CUDE_VPC_SIMS, CUDE_VPC_SELECT).
 * Options that shape the launch path take effect at the next cude_set_population_*.  No reference line: these are
 * properties of this implementation. */
int32_t cude_set_option(cude_ctx* ctx, const char* name, const char* value);

#ifdef __cplusplus
}
#endif
#endif /* CUDE_H */
