"""Every compiled tangent kernel (cude_sensitivity) and fit kernel (cude_refine_conditional), for every shape it is
compiled for -- on inputs whose biases are not zero (tests/adaptive_cases.py; tests/test_tangent_cases_host.py shows on the
oracle alone that a 1e-3 change of ANY network parameter moves sens, info and score by at least four of the bars below,
and which subjects of the fit cases are decided by rounding).  tests/test_gpu_sensitivity.py and tests/test_gpu_refine.py
run a handful of shapes on Glorot parameters, whose biases are zero.

Which kernel a call lands on is not observable through the engine; the dispatch rules, restated:

  cude_sensitivity (csrc/cude_sens.hip launch_cpep_sens / launch_supp_sens)
    fixed step (n_steps > 0)
      c-peptide   cpep_sens_kernel<Mlp<nin, w, d, 1>, n_state> for the 24 CUDE_CPEP_SHAPES, n_state 2 and 3;
                  with another activation pair cpep_sens_kernel<CpepNetG<nin, w, d, HA, OA>, n_state> for the 3
                  CUDE_CPEP_GENERAL_SHAPES x the 5 CUDE_GENERAL_ACTS
      suppression supp_sens_kernel<w, d, HA, OA>: the 16 CUDE_SUPP_SHAPES; the 2 CUDE_SUPP_GENERAL_SHAPES x 5 pairs
    adaptive (n_steps = 0, n_state 2)
      the one-body kernel adaptive_kernel<CpepAdTan<Net>> / adaptive_kernel<SuppAdTan<w, d>> on any grid -- whereas the
      GRADIENT launch of a c-peptide grid of at most five knots runs the team or the unrolled kernel.  On the six knots
      of TP6 both launches run the one-body kernel, so their accepted steps can be compared bit for bit.
  cude_refine_conditional, fixed step (csrc/cude_refine.hip launch_cpep_refine / launch_supp_refine)
    option "refine_fused" = 1 (the default): cpep_refine_kernel<Net> (one kernel for either n_state), CUDE_CPEP_SHAPES_0
      in translation unit 0, _1 and the general-activation shapes in 1, _2 in 2; supp_refine_kernel<w, d, HA, OA>
    "refine_fused" = 0: per evaluation one launch of the fixed-step tangent kernel above and one refine_step_kernel.

Compiled kernels reached:
  a. fixed-step tangent, tuned shapes           24 x 2 + 16 = 64 of 64
  b. fixed-step tangent, general activations    15 (n_state 2; the n_state 3 twins are not run) + 10 = 25 of 40
  c. adaptive tangent, tuned shapes             24 + 16 = 40 of 40 (general activations: not run)
  d. fused fits, tuned shapes                   24 + 16 = 40 of 40
  e. fused fits, general activations            15 + 10 = 25 of 25

Bars are the project's own -- _check_all of tests/test_gpu_sensitivity.py: 1e-9 of the reference array's max-norm
(GRAD_RTOL), 1e-10 for SSE, 1e-8 over the device's own adaptive steps (ADAPT_RTOL); X_BAR of tests/test_gpu_refine.py.
References: tests/sensitivity_ref.py (complex step on the oracle), tests/refine_ref.py (the rule restated).  Every figure
is printed before it is asserted (pytest -s shows them; DESIGN.md section 5 records the worst per group)."""
import numpy as np
import pytest

import adaptive_cases as ac
from test_gpu_refine import PEN, X_BAR
from test_gpu_sensitivity import ADAPT_RTOL, GRAD_RTOL, SSE_RTOL, _check_all

pytestmark = pytest.mark.gpu

CPEP_IDS = [str(a) for a in ac.CPEP_SHAPES]
SUPP_IDS = [str(s) for s in ac.SUPP_SHAPES]
ACT_IDS = ["-".join(a) for a in ac.GENERAL_ACTS]
MAX_EVALS = 2                                   # CUDE_REFINE_MAX_EVALS


def _ratios(tag, out, ref):
    """One line with error / max-norm of the reference for sens, info, score and the largest relative SSE error."""
    sens, info, score, sse = ref
    r = [float(np.max(np.abs(out[k] - w)) / np.max(np.abs(w))) for k, w in (("sens", sens), ("info", info), ("score", score))]
    print(f"{tag}: ratios sens {r[0]:.2e} info {r[1]:.2e} score {r[2]:.2e} sse {np.max(np.abs(out['sse'] - sse) / sse):.2e}")


def _engine(model, c, n_steps, n_state=None, acts=()):
    from cude.engine import Engine
    eng = Engine(model, c["arch"], n_steps=n_steps, n_state=n_state)
    if acts:
        eng.set_option("hidden_activation", acts[0])
        eng.set_option("output_activation", acts[1])
    if model == "cpep":
        eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
        eng.set_params(c["nn"], c["beta"])
    else:
        eng.set_population_supp(c["tp"], c["data"])
        eng.set_params(c["nn"], c["theta"])
    assert not eng.fallback_kernel
    return eng


def _reference(model, c, x, acts=(), n_state=2):
    """(sens, info, score, sse) of the fixed-step solve (30 steps) at the conditional parameters x."""
    import sensitivity_ref as ref
    arch = tuple(c["arch"]) + tuple(acts)
    if model == "cpep":
        return ref.cpep_sens(c["nn"], x, ac.cpep_population(c), arch, 30, n_state)
    return ref.supp_sens(c["nn"], x, c["data"], c["tp"], arch, 30)


# ----------------------------------------------------------------------------- a, b: fixed-step tangent
def _fixed(model, k, n_state, acts=()):
    c, cond, _ = ac.tangent_case(model, k)
    N = c[cond].size
    eng = _engine(model, c, 30, n_state, acts)
    out = eng.sensitivity()
    fwd = eng.forward(want_sse=True)
    assert eng.n_failed() == 0
    eng.close()
    assert out["sens"].shape == (n_state, len(c["tp"]), N)
    ref = _reference(model, c, c[cond], acts, n_state)
    _ratios(f"fixed {model} {c['arch']} {'-'.join(acts)} n_state {n_state} N {N}", out, ref)
    _check_all(out, ref, GRAD_RTOL)                                  # (column t_0 exactly 0 is part of it)
    if model == "supp":
        assert np.all(out["sens"][0] == 0.0)                         # state 1 depends on no parameter
    assert np.all(np.abs(out["sse"] - fwd["sse"]) <= SSE_RTOL * fwd["sse"])


@pytest.mark.parametrize("n_state", [2, 3])
@pytest.mark.parametrize("k", range(len(ac.CPEP_SHAPES)), ids=CPEP_IDS)
def test_cpep_fixed_step_tangent(k, n_state):
    _fixed("cpep", k, n_state)


@pytest.mark.parametrize("k", range(len(ac.SUPP_SHAPES)), ids=SUPP_IDS)
def test_supp_fixed_step_tangent(k):
    _fixed("supp", k, 3)


@pytest.mark.parametrize("acts", ac.GENERAL_ACTS, ids=ACT_IDS)
@pytest.mark.parametrize("shape", ac.CPEP_GENERAL_SHAPES, ids=str)
def test_cpep_fixed_step_tangent_general_activations(shape, acts):
    _fixed("cpep", ac.CPEP_SHAPES.index(shape), 2, acts)


@pytest.mark.parametrize("acts", ac.GENERAL_ACTS, ids=ACT_IDS)
@pytest.mark.parametrize("shape", ac.SUPP_GENERAL_SHAPES, ids=str)
def test_supp_fixed_step_tangent_general_activations(shape, acts):
    _fixed("supp", ac.SUPP_SHAPES.index(shape), 3, acts)


# ----------------------------------------------------------------------------- c: adaptive tangent
def _adaptive(model, k):
    import sensitivity_ref as ref
    if model == "cpep":
        arch = ac.CPEP_SHAPES[k]
        c = ac.cpep_case(arch, k, ac.TP6, ac.cpep_subjects(arch))
        N = c["beta"].size
    else:
        c, _, _ = ac.tangent_case("supp", k)
        N = c["theta"].size
    eng = _engine(model, c, 0, 2 if model == "cpep" else 3)
    eng.loss_grad()
    want = [eng.adaptive_steps(i) for i in range(N)]
    fwd = eng.forward(want_sse=True)
    out = eng.sensitivity()
    got = [eng.adaptive_steps(i) for i in range(N)]
    assert eng.n_failed() == 0
    eng.close()
    for (t0, d0), (t1, d1) in zip(want, got):                       # the accepted steps, bit for bit
        assert np.array_equal(t0, t1) and np.array_equal(d0, d1)
    print(f"adaptive {model} {c['arch']} N {N}: sse vs cude_forward {np.max(np.abs(out['sse'] - fwd['sse']) / fwd['sse']):.3e}, "
          f"{min(len(t) for t, _ in got)}..{max(len(t) for t, _ in got)} accepted steps")
    assert np.all(np.abs(out["sse"] - fwd["sse"]) <= 1e-14 * fwd["sse"])
    steps = [list(zip(t, dt)) for t, dt in got]
    if model == "cpep":
        r = ref.cpep_sens_replay(c["nn"], c["beta"], ac.cpep_population(c), c["arch"], steps)
    else:
        r = ref.supp_sens_replay(c["nn"], c["theta"], c["data"], c["tp"], c["arch"], steps)
        assert np.all(out["sens"][0] == 0.0)
    _ratios(f"adaptive {model} {c['arch']} N {N}", out, r)
    _check_all(out, r, ADAPT_RTOL, replay=True)


@pytest.mark.parametrize("k", range(len(ac.CPEP_SHAPES)), ids=CPEP_IDS)
def test_cpep_adaptive_tangent_six_knots(k):
    _adaptive("cpep", k)


@pytest.mark.parametrize("k", range(len(ac.SUPP_SHAPES)), ids=SUPP_IDS)
def test_supp_adaptive_tangent(k):
    _adaptive("supp", k)


# ----------------------------------------------------------------------------- d, e: fused fits
def _sse_at(eng, x):
    eng.set_params(None, x)
    return eng.forward(want_sse=True)["sse"]


def _one_evaluation(tag, model, c, eng, x0, box, acts=()):
    """max_evals = 1: the fit kernel's own instantiation of the sweep, evaluated once at the clamped start."""
    r1 = eng.refine_conditional(x0, *box, max_evals=1)
    x = np.clip(x0, *box)
    assert np.array_equal(r1["x"], x) and np.all(r1["evals"] == 1) and np.all(r1["status"] == MAX_EVALS)
    info = _reference(model, c, x, acts)[1]
    sse = _sse_at(eng, x)
    print(f"{tag} one evaluation: ratios info {np.max(np.abs(r1['info'] - info)) / np.max(info):.2e} "
          f"sse vs cude_forward {np.max(np.abs(r1['sse'] - sse) / sse):.2e}")
    assert np.max(np.abs(r1["info"] - info)) <= GRAD_RTOL * np.max(info)
    assert np.all(np.abs(r1["sse"] - sse) <= 1e-12 * sse)


def _fused_equals_stepped(tag, eng, x0, box):
    """Both forms evaluate through the one sweep of csrc/cude_tangent.h and judge by the one refine_update: bit for bit,
    every subject.  Returns the fused form's plain result."""
    plain = None
    for pw, pc in ((0.0, 0.0), PEN):
        out = []
        for fused in (1, 0):
            eng.set_option("refine_fused", fused)
            out.append(eng.refine_conditional(x0, *box, penalty_weight=pw, penalty_center=pc))
        eng.set_option("refine_fused", 1)
        a, b = out
        print(f"{tag} pw={pw} fused vs stepped: x differs for {np.count_nonzero(a['x'] != b['x'])}, evals for "
              f"{np.count_nonzero(a['evals'] != b['evals'])}, status for {np.count_nonzero(a['status'] != b['status'])} "
              f"of {x0.size}; evals {a['evals'].min()}..{a['evals'].max()}, status {np.bincount(a['status'], minlength=5)}")
        assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["evals"], b["evals"]) and np.array_equal(a["status"], b["status"])
        plain = a if plain is None else plain
    return plain


def _fit(model, k):
    s = ac.fit_study(model, k)
    c, x0, box, want, ok = s["case"], s["x0"], s["box"], s["ref"], s["admissible"]
    tag = f"fit {model} {c['arch']} N {x0.size}"
    eng = _engine(model, c, 30, 2 if model == "cpep" else 3)
    _one_evaluation(tag, model, c, eng, x0, box)
    got = _fused_equals_stepped(tag, eng, x0, box)
    # the default call against the restatement, on the subjects that rounding does not decide
    dx = np.abs(got["x"] - want["x"]) / (1 + np.abs(want["x"]))
    print(f"{tag} vs the restatement: {np.count_nonzero(ok)} admissible; max |dx|/(1+|x|) {dx[ok].max():.2e} "
          f"({dx[ok].max() / X_BAR:.2e} of the bar), evals differ for {np.count_nonzero((got['evals'] != want['evals'])[ok])}, "
          f"status for {np.count_nonzero((got['status'] != want['status'])[ok])}")
    assert np.all(dx[ok] <= X_BAR)
    assert np.array_equal(got["status"][ok], want["status"][ok]) and np.array_equal(got["evals"][ok], want["evals"][ok])
    # the outputs belong to the returned point (every subject)
    sse = _sse_at(eng, got["x"])
    info = eng.sensitivity(want_sens=False)["info"]
    print(f"{tag} outputs: sse vs cude_forward {np.max(np.abs(got['sse'] - sse) / sse):.2e}, "
          f"info vs cude_sensitivity {np.max(np.abs(got['info'] - info)) / np.max(info):.2e}")
    assert np.all(np.abs(got["sse"] - sse) <= 1e-12 * sse)
    assert np.max(np.abs(got["info"] - info)) <= 1e-9 * np.max(info)
    assert eng.n_failed() == 0
    eng.close()


@pytest.mark.parametrize("k", range(len(ac.CPEP_SHAPES)), ids=CPEP_IDS)
def test_cpep_fused_fit(k):
    _fit("cpep", k)


@pytest.mark.parametrize("k", range(len(ac.SUPP_SHAPES)), ids=SUPP_IDS)
def test_supp_fused_fit(k):
    _fit("supp", k)


def _fit_general(model, k, acts):
    """Checks 1 and 3 of _fit: under relu the objective is not smooth, so the restatement's admissibility rule does not
    apply; the two device forms still share every evaluation."""
    c, cond, box = ac.tangent_case(model, k)
    tag = f"fit {model} {c['arch']} {'-'.join(acts)} N {c[cond].size}"
    eng = _engine(model, c, 30, 2 if model == "cpep" else 3, acts)
    _one_evaluation(tag, model, c, eng, c[cond], box, acts)
    _fused_equals_stepped(tag, eng, c[cond], box)
    eng.close()


@pytest.mark.parametrize("acts", ac.GENERAL_ACTS, ids=ACT_IDS)
@pytest.mark.parametrize("shape", ac.CPEP_GENERAL_SHAPES, ids=str)
def test_cpep_fused_fit_general_activations(shape, acts):
    _fit_general("cpep", ac.CPEP_SHAPES.index(shape), acts)


@pytest.mark.parametrize("acts", ac.GENERAL_ACTS, ids=ACT_IDS)
@pytest.mark.parametrize("shape", ac.SUPP_GENERAL_SHAPES, ids=str)
def test_supp_fused_fit_general_activations(shape, acts):
    _fit_general("supp", ac.SUPP_SHAPES.index(shape), acts)
