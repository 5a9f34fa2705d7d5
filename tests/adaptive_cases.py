"""Inputs for the per-shape tests of the adaptive Tsit5 kernels (tests/test_gpu_adaptive_shapes.py on the device,
tests/test_adaptive_cases_host.py for the inputs themselves), and the shape lists those tests walk.

Which kernel an adaptive launch (cude_config.n_steps = 0) lands on -- csrc/cude_adaptive.hip launch_cpep_adaptive /
launch_supp_adaptive, restated:

  c-peptide, tanh / softplus network of one of the 24 CPEP_SHAPES, T knots in the glucose grid:
    T <= 5 (kUnrolledKnots)
        * shape in TEAM_SHAPES, option "adaptive_team" = 1 (the default) and at most 256 (kTeamMaxWaves) single-wave
          workgroups in the launch, ceil(N / 64) x parameter sets: the TEAM kernel (cude_adaptive_team.hip, five or six
          waves over 64 subjects) -- except the GRADIENT launch of a network with more than 64 gradient accumulators,
          (2,8,2) and (2,7,2) of the team's shapes, which goes on to
        * the UNROLLED one-wave kernel (cude_adaptive_unrolled.hip, all 24 shapes): everything else on T <= 5, i.e.
          "adaptive_team" = 0, the 16 shapes outside TEAM_SHAPES, larger launches.
    6 <= T <= 32 (kMaxObs)
        * the ONE-BODY kernel (cude_adaptive_body.h), instantiated in three translation units: CPEP_SHAPES[0:8] in
          cude_adaptive.hip, [8:16] in launch_cpep_adaptive_part1, [16:24] in launch_cpep_adaptive_part2.
          "adaptive_team" plays no part.
  suppression, (4, w, d):
        * (w, d) in SUPP_UNROLLED: the unrolled kernel (cude_adaptive_unrolled_supp.hip);
        * the other 12 SUPP_SHAPES: the one-body kernel (cude_adaptive.hip).

So, with the cases below: cpep_case(arch, k, TP5, N) with N <= 70 and up to three parameter sets (at most six workgroups)
reaches the team kernel for TEAM_SHAPES on an engine with "adaptive_team" = 1 and the unrolled kernel on one with
"adaptive_team" = 0 or for any other shape; cpep_case(arch, k, TP6, N) -- TP6 is the smallest grid that leaves the
unrolled kernels -- reaches the one-body kernel for every shape; supp_case reaches the unrolled suppression kernel for
SUPP_UNROLLED and the one-body kernel otherwise.  Which kernel ran is not observable through the engine: the tests rely
on this rule, and tests/test_adaptive_cases_host.py holds the lists here to the headers the rule is written in.

Why not conftest.make_cpep_case / make_supp_case: cude_oracle.glorot_params gives the tuned shapes ZERO biases, so a
forward pass through them never reads a non-zero bias (a kernel that fetched bias j + 1 for unit j would pass), and the
three-input shapes see raw ages of 20 ... 79 on Glorot-scale weights, which saturates the first layer and leaves its
weights' gradients 1e-15 ... 1e-22 of the largest entry -- invisible at a max-norm tolerance.  biased_params() gives every
bias a value and scales the age column; tests/test_adaptive_cases_host.py asserts on the oracle alone that with these
inputs every layer's weight block and bias block of the gradient is within 1e3 of the largest, that the solves take a
sensible number of steps, and that no accept / reject decision sits on the threshold."""
import numpy as np

import cude_oracle as o

# csrc/cude_shapes.h CUDE_CPEP_SHAPES_0 / _1 / _2 and CUDE_SUPP_SHAPES, in their order
CPEP_SHAPES = [(2, 4, 2), (2, 6, 2), (3, 4, 2), (2, 8, 2), (2, 4, 3), (2, 3, 2), (2, 5, 2), (2, 7, 2),
               (3, 6, 2), (2, 4, 1), (2, 6, 1), (2, 6, 3), (2, 8, 1), (2, 8, 3), (3, 8, 2), (2, 3, 1),
               (2, 5, 1), (2, 7, 1), (2, 3, 3), (2, 5, 3), (2, 7, 3), (3, 4, 1), (3, 6, 1), (3, 4, 3)]
SUPP_SHAPES = [(3, 5), (3, 2), (4, 2), (6, 2), (5, 2), (3, 3), (8, 2), (3, 4), (4, 3), (4, 4), (5, 3), (6, 3), (3, 1), (4, 1),
               (6, 1), (8, 1)]
TEAM_SHAPES = CPEP_SHAPES[:8]                           # CUDE_CPEP_SHAPES_0
SUPP_UNROLLED = [(3, 5), (3, 3), (3, 4), (3, 2)]        # csrc/cude_shapes.h CUDE_SUPP_AD_UNROLLED
TWO_WORKGROUPS = [(2, 4, 2), (3, 6, 2), (2, 5, 1)]      # first shape of each group: run with 70 subjects (a second
                                                        # workgroup, a wave of six lanes), the others with 16
SUPP_TWO_WORKGROUPS = [(3, 5), (4, 3), (3, 1)]          # the same for the tangent and fit kernels of the suppression model
                                                        # (tests/test_gpu_tangent_shapes.py): 70 subjects, the others 12
# csrc/cude_shapes.h CUDE_CPEP_GENERAL_SHAPES / CUDE_SUPP_GENERAL_SHAPES: the shapes that are also compiled with the
# activation pairs of CUDE_GENERAL_ACTS, here as (hidden, output) names in its order (csrc/cude_kernels.h kActHidden* /
# kActOut*: hidden 0 tanh, 1 relu, 2 sigmoid; output 0 softplus, 1 identity)
CPEP_GENERAL_SHAPES = [(2, 4, 2), (2, 6, 2), (3, 4, 2)]
SUPP_GENERAL_SHAPES = [(3, 5), (3, 3)]
GENERAL_ACTS = [("tanh", "identity"), ("relu", "softplus"), ("relu", "identity"), ("sigmoid", "softplus"),
                ("sigmoid", "identity")]

TP5 = [0.0, 30.0, 60.0, 90.0, 120.0]
TP6 = [0.0, 15.0, 30.0, 60.0, 90.0, 120.0]


def cpep_subjects(arch):
    return 70 if tuple(arch) in TWO_WORKGROUPS else 16


def supp_subjects(shape):
    return 70 if tuple(shape) in SUPP_TWO_WORKGROUPS else 12


def layer_blocks(arch):
    """[(name, slice)] of the parameter vector in the layout of cude_oracle.mlp: per layer the weights (column-major),
    then the biases."""
    nin, w, d = arch[:3]
    out, off, fan = [], 0, nin
    for l in range(d):
        out.append((f"W{l + 1}", slice(off, off + w * fan)))
        out.append((f"b{l + 1}", slice(off + w * fan, off + w * fan + w)))
        off += w * fan + w
        fan = w
    out.append(("Wout", slice(off, off + fan)))
    out.append(("bout", slice(off + fan, off + fan + 1)))
    return out


def bias_index(arch):
    return np.concatenate([np.arange(s.start, s.stop) for name, s in layer_blocks(arch) if name.startswith("b")])


def biased_params(arch, seed):
    """glorot_params with every bias drawn from 0.2 N(0, 1) and, for the three-input shapes, the first layer's age column
    (nn[2w:3w]) divided by 50, so that ages of 20 ... 79 reach the first layer at the scale of its other inputs."""
    nn = o.glorot_params(arch, seed).copy()
    rng = np.random.default_rng([int(seed), 0xB1A5])
    idx = bias_index(arch)
    nn[idx] = 0.2 * rng.standard_normal(idx.size)
    if arch[0] == 3:
        w = arch[1]
        nn[2 * w:3 * w] /= 50.0
    return nn


def cpep_case(arch, k, tp, N):
    """Seeded c-peptide population on the grid `tp` (the recipe of test_cpep_adaptive_other_sampling_grids) with
    biased_params; k = the shape's position in CPEP_SHAPES."""
    rng = np.random.default_rng(100 + k)
    tp = np.array(tp, dtype=np.float64)
    age, t2 = rng.uniform(20, 79, N), rng.random(N) < 0.4
    G = 5.0 + np.abs(rng.standard_normal((N, tp.size))).cumsum(1)
    obs = 0.5 + rng.random((N, tp.size))
    beta = rng.normal(-0.6, 0.5, N)
    return dict(tp=tp, G=G, obs=obs, age=age, t2dm=t2, nn=biased_params(arch, 9 + k), beta=beta, arch=tuple(arch))


def cpep_population(c):
    return o.CPepPopulation(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"], covariate=(c["arch"][0] == 3))


def supp_case(shape, k, N):
    """conftest.make_supp_case's data with seed 7 + k and biased_params; shape = (w, d), k = its position in
    SUPP_SHAPES."""
    arch = (4,) + tuple(shape)
    seed = 7 + k
    rng = np.random.default_rng(seed)
    T = 8
    tp = np.linspace(0.0, 30.0, T)
    t = tp[None, :, None]
    kk = 0.3 + 0.2 * rng.random((1, 1, N))
    data = np.empty((3, T, N))
    data[0] = (10.0 * np.exp(-0.4 * t))[0]
    data[1] = (6.0 * t * np.exp(-kk * t) / 3.0)[0] + 0.2
    data[2] = (4.0 * (1 - np.exp(-0.15 * t)) * np.exp(-0.02 * t))[0] + 0.1
    data *= 1.0 + 0.1 * rng.standard_normal(data.shape)
    data = np.maximum(data, 0.0)
    data[0, 0] = 10.0 * (1 + 0.05 * rng.standard_normal(N))
    theta = 0.5 * rng.standard_normal(N)
    return dict(tp=tp, data=data, nn=biased_params(arch, seed + 1), theta=theta, arch=arch)


# ----------------------------------------------------------------------------- the oracle's own adaptive solves
class _Decisions(list):
    """`record` list for cude_oracle.solve_adaptive that also notes, at every accepted step, how many right-hand sides
    had been evaluated: a trial step costs six (stages 2 ... 7) after the two of the initial-step heuristic, so the note
    gives the index of the accepted trial and with it the whole accept / reject sequence."""

    def __init__(self, calls):
        super().__init__()
        self.calls, self.at = calls, []

    def append(self, item):
        super().append(item)
        self.at.append((self.calls[0] - 2) // 6 - 1)


def _solve(rhs, u0, tp, tol_scale):
    calls = [0]

    def counted(t, u):
        calls[0] += 1
        return rhs(t, u)
    rec = _Decisions(calls)
    out = o.solve_adaptive(counted, u0, tp, abstol=1e-6 * tol_scale, reltol=1e-3 * tol_scale, record=rec)
    n_trials = (calls[0] - 2) // 6
    accepted = set(rec.at)
    return out, list(rec), tuple(q in accepted for q in range(n_trials))


def cpep_solve(c, pop, i, tol_scale=1.0):
    """(outputs or None, [(t_n, dt_n)] of the accepted steps, (accepted?) per trial step) of subject i's solve."""
    c0 = float(pop.c0[i])
    return _solve(o.cpep_rhs_scalar(pop, i, c["nn"], float(np.exp(c["beta"][i])), c["arch"]),
                  [c0, float(pop.k2[i] / pop.k1[i]) * c0], pop.timepoints, tol_scale)


def supp_solve(s, i, tol_scale=1.0):
    import math
    p, et = [float(v) for v in s["nn"]], math.exp(float(s["theta"][i]))
    return _solve(lambda t, u: o.supp_rhs(math, p, et, s["arch"], t, u), [float(v) for v in s["data"][:, 0, i]],
                  [float(v) for v in s["tp"]], tol_scale)


def same_steps(rec, t, dt, span, tol):
    """The criterion of tests/test_gpu_adaptive_grad.py: as many accepted steps and every dt within tol of the span."""
    return len(rec) == len(t) and np.max(np.abs(np.array(rec)[:, 1] - dt)) <= tol * span


def block_ratios(g, arch):
    """{block: max-norm of the block of g / max-norm of g} over layer_blocks: each layer's weights and its biases."""
    top = np.max(np.abs(g))
    return {name: float(np.max(np.abs(g[s])) / top) for name, s in layer_blocks(arch)}


# ----------------------------------------------------------------------------- the tangent and fit kernels' cases
# (tests/test_gpu_tangent_shapes.py on the device, tests/test_tangent_cases_host.py for the inputs themselves)
CPEP_BOX, SUPP_BOX = (-4.0, 3.0), (-6.0, 4.0)           # the boxes of tests/test_gpu_refine.py
FIT_PERTURBATION = 1e-9                                 # the error the tangent kernels are allowed (GRAD_RTOL)


def tangent_case(model, k):
    """The fixed-step case of shape k of CPEP_SHAPES (model "cpep": five knots, 70 / 16 subjects) or SUPP_SHAPES ("supp":
    70 / 12 subjects) -> (case, name of its conditional parameter, box of its fits)."""
    if model == "cpep":
        arch = CPEP_SHAPES[k]
        return cpep_case(arch, k, TP5, cpep_subjects(arch)), "beta", CPEP_BOX
    shape = SUPP_SHAPES[k]
    return supp_case(shape, k, supp_subjects(shape)), "theta", SUPP_BOX


_FIT_STUDIES = {}


def fit_study(model, k, n_steps=30):
    """The perturbation rule of tests/test_gpu_refine.py / test_refine_host.py on tangent_case(model, k): the restatement
    tests/refine_ref.py from x0 = the case's conditional parameters (max_step 0.5, xtol 1e-7, 40 evaluations), and again
    with every info and score multiplied by 1 +- 1e-9 in the four sign combinations.  The five runs are ONE call of the
    restatement on the population repeated five times (no quantity crosses subjects; the suppression loss's weights are
    those of the population itself).  Returns dict(case, x0, box, ref = the unperturbed run's dict(x, objective, sse,
    info, evals, status), admissible (N,) bool: neither status nor evals changes in any of the four); computed once per
    shape."""
    if (model, k) in _FIT_STUDIES:
        return _FIT_STUDIES[model, k]
    import refine_ref as rr
    import sensitivity_ref as ref
    c, cond, box = tangent_case(model, k)
    x0, arch, nn = c[cond], c["arch"], c["nn"]
    N, f = x0.size, FIT_PERTURBATION
    combos = [(1.0, 1.0), (1 + f, 1 + f), (1 + f, 1 / (1 + f)), (1 - f, 1 - f), (1 - f, 1 / (1 - f))]     # (info, score)
    R = len(combos)
    f_info, f_score = (np.repeat([q[j] for q in combos], N) for j in (0, 1))
    if model == "cpep":
        pop = o.CPepPopulation(c["tp"], np.tile(c["G"], (R, 1)), np.tile(c["obs"], (R, 1)), np.tile(c["age"], R),
                               np.tile(c["t2dm"], R), covariate=(arch[0] == 3))

        def ev(x):
            with np.errstate(all="ignore"):
                _, info, score, sse = ref.cpep_sens(nn, x, pop, arch, n_steps, 2)
            return info * f_info, score * f_score, sse
    else:
        data, w2 = np.tile(c["data"], (1, 1, R)), 1.0 / o.supp_scale(c["data"]) ** 2

        def ev(x):
            with np.errstate(all="ignore"):
                u = ref._stack(o.supp_forward(np, nn, np.asarray(x, dtype=np.complex128) + 1j * ref.H, data, c["tp"], arch,
                                              n_steps), R * N)
                info, score, sse = ref._summaries(u, data, w2)
            return info * f_info, score * f_score, sse
    r = rr.refine(ev, np.tile(x0, R), *box, max_evals=40, xtol=1e-7, max_step=0.5)
    runs = {key: v.reshape(R, N) for key, v in r.items()}
    admissible = np.all((runs["status"] == runs["status"][0]) & (runs["evals"] == runs["evals"][0]), axis=0)
    out = dict(case=c, x0=x0, box=box, ref={key: v[0].copy() for key, v in runs.items()}, admissible=admissible)
    _FIT_STUDIES[model, k] = out
    return out
