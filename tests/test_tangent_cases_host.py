"""The inputs of tests/test_gpu_tangent_shapes.py (tests/adaptive_cases.py: tangent_case, fit_study, the general-activation
lists) are adequate -- shown on the CPU oracle alone (tests/sensitivity_ref.py, tests/refine_ref.py), so that they cannot
degrade without a test saying so.

(a) Visibility.  Every network parameter of every tuned shape, scaled by 1 + 1e-3, moves each of sens, info and score of
    the fixed-step tangent solve (30 steps) by at least 4e-9 of the array's max-norm = 4 x the device test's bar.  A
    kernel that misreads a weight or a bias errs by order 1 in that parameter, not 1e-3: more than 1000 bars.  (All P
    perturbed networks of a shape are solved in one batched call of the oracle; its unperturbed row is held to the
    reference helper's own result.)  Measured when this was written (the smallest move over the parameters, the three arrays and the shapes of a model):
        c-peptide    1.3e-8  ((2, 7, 3), parameter 115, sens)            every other shape >= 5.1e-8
        suppression  4.7e-9  ((8, 1),    parameter 37,  info)            every other shape >= 3.9e-8
    A case that falls below the bar gets another seed, the bar stays.
(b) Admissibility of the fit cases (adaptive_cases.fit_study, the rule of tests/test_refine_host.py): a subject whose status
    or evals changes when every info and score is multiplied by 1 +- 1e-9 is decided by rounding and is left out of the
    device test's comparison of x, status and evals.  Measured: 3 of 912 subjects -- one each of (2, 5, 3), (3, 4, 3) and
    suppression (3, 4) -- and none of the 420 subjects of the six 70-subject cases.  Asserted: at most ceil(N / 12) per
    shape, at most 2 % over all shapes; every subject takes between 4 and 40 evaluations and none ends FAILED or FLAT,
    so that score and info both steer every result.
(c) The general-activation cases: complex step against autograd, as tests/test_sensitivity_host.py does for the default
    pair -- a relu kink hit by an input would show as a disagreement."""
import math

import numpy as np
import pytest

import cude_oracle as o
import adaptive_cases as ac

VISIBLE = 4e-9                  # 4 x GRAD_RTOL of tests/test_gpu_tangent_shapes.py
SELF_TOL = 1e-12                # tests/test_sensitivity_host.py
CPEP_IDS = [str(a) for a in ac.CPEP_SHAPES]
SUPP_IDS = [str(s) for s in ac.SUPP_SHAPES]


def _sens(model, c, nn, acts=()):
    import sensitivity_ref as ref
    arch = tuple(c["arch"]) + tuple(acts)
    if model == "cpep":
        return ref.cpep_sens(nn, c["beta"], ac.cpep_population(c), arch, 30, 2)
    return ref.supp_sens(nn, c["theta"], c["data"], c["tp"], arch, 30)


# ----------------------------------------------------------------------------- (a) visibility
def _sens_of_many_networks(model, c, networks):
    """sensitivity_ref.cpep_sens / supp_sens (30 steps) for Q networks in one solve: networks (Q, P) -> sens (Q, n_state, T,
    N), info (Q, N), score (Q, N).  cude_oracle.mlp indexes the parameter vector along its first axis, so parameters of
    shape (P, Q, 1) broadcast against the subjects; every operation is elementwise, so row q is the solve of network q."""
    import sensitivity_ref as ref
    p = np.asarray(networks, dtype=np.float64).T[:, :, None]
    Q = p.shape[1]
    if model == "cpep":
        pop = ac.cpep_population(c)
        N, data, w2, observed = pop.N, pop.cpeptide.T[None], np.ones(1), slice(0, 1)
        traj = o.cpep_forward(np, p, c["beta"] + 1j * ref.H, pop, c["arch"], 30, 2)
    else:
        N, data, w2, observed = c["theta"].size, c["data"], 1.0 / o.supp_scale(c["data"]) ** 2, slice(0, 3)
        traj = o.supp_forward(np, p, c["theta"] + 1j * ref.H, c["data"], c["tp"], c["arch"], 30)
    u = np.array([[np.broadcast_to(np.asarray(traj[ti][s], dtype=np.complex128), (Q, N)) for ti in range(len(traj))]
                  for s in range(len(traj[0]))]).transpose(2, 0, 1, 3)
    sens = u.imag / ref.H
    d, r = sens[:, observed], u.real[:, observed] - data
    w2 = w2[:, None, None]
    return sens, (w2 * d ** 2).sum(axis=(1, 2)), (w2 * r * d).sum(axis=(1, 2))


def _visibility(model, k):
    c, _, _ = ac.tangent_case(model, k)
    P = c["nn"].size
    networks = np.tile(c["nn"], (P + 1, 1))                          # row 0: the case's own; row 1 + p: parameter p scaled
    networks[1 + np.arange(P), np.arange(P)] *= 1.0 + 1e-3
    many = _sens_of_many_networks(model, c, networks)
    base = _sens(model, c, c["nn"])[:3]
    worst = (np.inf, None, None)
    for name, a, b in zip(("sens", "info", "score"), many, base):
        top = np.max(np.abs(b))
        assert np.all(np.isfinite(a)) and top > 0.0
        assert np.max(np.abs(a[0] - b)) <= SELF_TOL * top, name     # the batched solve is the reference helper's
        moves = np.max(np.abs(a[1:] - b).reshape(P, -1), axis=1) / top
        worst = min(worst, (float(moves.min()), int(moves.argmin()), name))
    print(f"{model} {c['arch']}: smallest move {worst[0]:.2e} of the max-norm ({worst[2]}, parameter {worst[1]})")
    assert worst[0] >= VISIBLE, worst


@pytest.mark.parametrize("k", range(len(ac.CPEP_SHAPES)), ids=CPEP_IDS)
def test_every_parameter_is_visible_cpep(k):
    _visibility("cpep", k)


@pytest.mark.parametrize("k", range(len(ac.SUPP_SHAPES)), ids=SUPP_IDS)
def test_every_parameter_is_visible_supp(k):
    _visibility("supp", k)


# ----------------------------------------------------------------------------- (b) admissibility of the fit cases
def _admissible(model, k):
    import refine_ref as rr
    s = ac.fit_study(model, k)
    r, N = s["ref"], s["x0"].size
    bad = int(np.count_nonzero(~s["admissible"]))
    print(f"{model} {s['case']['arch']}: {bad} of {N} inadmissible, evals {r['evals'].min()}..{r['evals'].max()}, "
          f"status {np.bincount(r['status'], minlength=5)}")
    assert np.all((s["x0"] > s["box"][0]) & (s["x0"] < s["box"][1]))          # the clamped start is the start
    assert bad <= math.ceil(N / 12)
    assert r["evals"].min() >= 4 and r["evals"].max() <= 40
    assert not np.any(np.isin(r["status"], [rr.FAILED, rr.FLAT]))


@pytest.mark.parametrize("k", range(len(ac.CPEP_SHAPES)), ids=CPEP_IDS)
def test_fit_case_is_admissible_cpep(k):
    _admissible("cpep", k)


@pytest.mark.parametrize("k", range(len(ac.SUPP_SHAPES)), ids=SUPP_IDS)
def test_fit_case_is_admissible_supp(k):
    _admissible("supp", k)


def test_inadmissible_share_over_all_shapes():
    """Reads what the per-shape tests computed (and computes it when run on its own)."""
    studies = [ac.fit_study("cpep", k) for k in range(len(ac.CPEP_SHAPES))] + \
              [ac.fit_study("supp", k) for k in range(len(ac.SUPP_SHAPES))]
    bad = sum(int(np.count_nonzero(~s["admissible"])) for s in studies)
    total = sum(s["x0"].size for s in studies)
    big = [s for s in studies if s["x0"].size == 70]
    print(f"inadmissible: {bad} of {total}; in the 70-subject cases {sum(int(np.count_nonzero(~s['admissible'])) for s in big)} "
          f"of {70 * len(big)}")
    assert total == 21 * 16 + 3 * 70 + 13 * 12 + 3 * 70 and len(big) == 6
    assert bad <= 0.02 * total


@pytest.mark.parametrize("model,k", [("cpep", 5), ("supp", 7)])
def test_the_study_run_of_five_is_five_runs_of_one(model, k):
    """fit_study evaluates the population repeated five times in one call of the restatement: its unperturbed fifth is,
    bit for bit, the restatement over tests/refine_ref.py's own evaluator on the population itself, and its mask is the
    one the four perturbed runs give one by one (suppression (3, 4) has an inadmissible subject)."""
    import refine_ref as rr
    s = ac.fit_study(model, k)
    c = s["case"]
    make = (lambda **kw: rr.cpep_evaluator(c, **kw)) if model == "cpep" else (lambda **kw: rr.supp_evaluator(c, **kw))
    base = rr.refine(make(), s["x0"], *s["box"])
    for key in ("x", "objective", "sse", "info", "evals", "status"):
        assert np.array_equal(base[key], s["ref"][key]), key
    same = np.ones(s["x0"].size, bool)
    f = ac.FIT_PERTURBATION
    for fi, fs in ((1 + f, 1 + f), (1 + f, 1 / (1 + f)), (1 - f, 1 - f), (1 - f, 1 / (1 - f))):
        r = rr.refine(make(f_info=fi, f_score=fs), s["x0"], *s["box"])
        same &= (r["status"] == base["status"]) & (r["evals"] == base["evals"])
    assert np.array_equal(same, s["admissible"])


# ----------------------------------------------------------------------------- (c) the general-activation cases
def _general(model, shape, acts):
    import sensitivity_ref as ref
    if model == "cpep":
        k = ac.CPEP_SHAPES.index(shape)
        c, _, _ = ac.tangent_case("cpep", k)
        arch = shape + acts
        st = ref.cpep_sens_torch(c["nn"], c["beta"], ac.cpep_population(c), arch, 30, 2)
    else:
        k = ac.SUPP_SHAPES.index(shape)
        c, _, _ = ac.tangent_case("supp", k)
        st = ref.supp_sens_torch(c["nn"], c["theta"], c["data"], c["tp"], c["arch"] + acts, 30)
    sens, info, score, sse = _sens(model, c, c["nn"], acts)
    err = float(np.max(np.abs(sens - st)) / np.max(np.abs(sens)))
    print(f"{model} {shape} {acts}: complex step vs autograd {err:.2e}; info {info.min():.2e}..{info.max():.2e}")
    assert np.all(np.isfinite(sens)) and np.all(np.isfinite(sse)) and np.all(sens[:, 0] == 0.0)
    assert err <= SELF_TOL
    assert np.count_nonzero(info) >= info.size // 2               # (relu may switch a subject's production off)


@pytest.mark.parametrize("acts", ac.GENERAL_ACTS, ids=["-".join(a) for a in ac.GENERAL_ACTS])
@pytest.mark.parametrize("shape", ac.CPEP_GENERAL_SHAPES, ids=str)
def test_general_activation_case_cpep(shape, acts):
    _general("cpep", shape, acts)


@pytest.mark.parametrize("acts", ac.GENERAL_ACTS, ids=["-".join(a) for a in ac.GENERAL_ACTS])
@pytest.mark.parametrize("shape", ac.SUPP_GENERAL_SHAPES, ids=str)
def test_general_activation_case_supp(shape, acts):
    _general("supp", shape, acts)
