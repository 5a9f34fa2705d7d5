"""Every compiled order-2 forward-mode kernel (cude_curvature, csrc/cude_curv.hip), for every shape it is compiled for, on
the inputs of tests/test_gpu_tangent_shapes.py (adaptive_cases.tangent_case: live biases, N = 70 / 16 / 12, 30 steps).

The dispatch is cude_sensitivity's (csrc/cude_curv.hip launch_cpep_curv / launch_supp_curv), restated:
  fixed step   cpep_curv_kernel<Mlp<nin, w, d, 1>, n_state> for the 24 CUDE_CPEP_SHAPES, n_state 2 and 3;
               cpep_curv_kernel<CpepNetG<...>, n_state> for the 3 general shapes x 5 activation pairs;
               supp_curv_kernel<w, d, HA, OA>: the 16 CUDE_SUPP_SHAPES; the 2 general shapes x 5 pairs
  adaptive     adaptive_kernel<CpepAdCurv<Net>> / adaptive_kernel<SuppAdCurv<w, d>> (n_state 2; tuned shapes only)

Compiled kernels reached: fixed-step tuned 24 x 2 + 16 = 64 of 64; fixed-step general activations 15 (n_state 2) + 10 = 25
of 40; adaptive 24 + 16 = 40 of 40.

Bars are the project's own (tests/test_gpu_sensitivity.py): GRAD_RTOL = 1e-9 of the reference array's max-norm for sens2 and
curv in fixed-step mode, ADAPT_RTOL = 1e-8 over the device's own adaptive steps, SSE_RTOL for sse.  info, score and sse are
held to the same references as cude_sensitivity, and to cude_sensitivity's own outputs on the same engine within twice
those bars.  References: tests/curvature_ref.py -- route (b) (stencil over complex-step first derivatives; held to route
(a) at 1e-10 by tests/test_curvature_host.py), route (a) (torch double backward) for the relu cases, where a stencil
straddles kinks.  Every ratio is printed before it is asserted (pytest -s; DESIGN.md section 5 records the worst per
group)."""
import numpy as np
import pytest

import adaptive_cases as ac
from test_gpu_sensitivity import ADAPT_RTOL, GRAD_RTOL, SSE_RTOL
from test_gpu_tangent_shapes import _engine

pytestmark = pytest.mark.gpu

CPEP_IDS = [str(a) for a in ac.CPEP_SHAPES]
SUPP_IDS = [str(s) for s in ac.SUPP_SHAPES]
ACT_IDS = ["-".join(a) for a in ac.GENERAL_ACTS]

_REFS = {}


def _reference(model, k, acts=(), n_state=2):
    """curvature_ref's dict for the fixed-step case (30 steps), computed once per case."""
    key = (model, k, tuple(acts), n_state)
    if key not in _REFS:
        import curvature_ref as cr
        c, cond, _ = ac.tangent_case(model, k)
        arch = tuple(c["arch"]) + tuple(acts)
        relu = "relu" in acts
        if model == "cpep":
            f = cr.cpep_curv_torch if relu else cr.cpep_curv
            _REFS[key] = f(c["nn"], c[cond], ac.cpep_population(c), arch, 30, n_state)
        else:
            f = cr.supp_curv_torch if relu else cr.supp_curv
            _REFS[key] = f(c["nn"], c[cond], c["data"], c["tp"], arch, 30)
    return _REFS[key]


def _check(tag, out, sens_out, ref, rtol, replay=False):
    """out: Engine.curvature(); sens_out: Engine.sensitivity() on the same engine; ref: curvature_ref's dict."""
    def ratio(a, b):
        return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
    r = {k: ratio(out[k], ref[k]) for k in ("sens2", "curv", "info", "score")}
    sse_rel = float(np.max(np.abs(out["sse"] - ref["sse"]) / ref["sse"]))
    sse_top = float(np.max(np.abs(out["sse"] - ref["sse"])) / np.max(ref["sse"]))
    own = {k: ratio(out[k], sens_out[k]) for k in ("info", "score")}
    own_sse = float(np.max(np.abs(out["sse"] - sens_out["sse"]) / sens_out["sse"]))
    print(f"{tag}: ratios sens2 {r['sens2']:.2e} curv {r['curv']:.2e} info {r['info']:.2e} score {r['score']:.2e} "
          f"sse {sse_rel:.2e} (of the largest {sse_top:.2e}); vs cude_sensitivity info {own['info']:.2e} "
          f"score {own['score']:.2e} sse {own_sse:.2e}")
    for k in ("sens2", "curv", "info", "score"):
        assert r[k] <= rtol, (k, r[k])
    if replay:
        assert sse_top <= SSE_RTOL
    else:
        assert sse_rel <= SSE_RTOL
    assert own["info"] <= 2 * rtol and own["score"] <= 2 * rtol and own_sse <= 2 * SSE_RTOL
    assert np.all(out["sens2"][:, 0, :] == 0.0)                     # column t_0 is exactly 0
    # the identity of rule 3, on the device's own numbers: curv - info is the second-order sum
    second = ref["second"]
    assert np.max(np.abs((out["curv"] - out["info"]) - second)) <= 2 * rtol * max(np.max(np.abs(ref["curv"])), np.max(ref["info"]))


# ----------------------------------------------------------------------------- fixed step
def _fixed(model, k, n_state, acts=()):
    c, cond, _ = ac.tangent_case(model, k)
    N = c[cond].size
    eng = _engine(model, c, 30, n_state, acts)
    nn0, cond0 = eng.get_params()
    out = eng.curvature()
    sens_out = eng.sensitivity(want_sens=False)
    assert eng.n_failed() == 0
    nn1, cond1 = eng.get_params()
    eng.close()
    assert np.array_equal(nn0, nn1) and np.array_equal(cond0, cond1)
    assert out["sens2"].shape == (n_state, len(c["tp"]), N)
    ref = _reference(model, k, acts, n_state)
    _check(f"fixed {model} {c['arch']} {'-'.join(acts)} n_state {n_state} N {N}", out, sens_out, ref, GRAD_RTOL)
    if model == "supp":
        assert np.all(out["sens2"][0] == 0.0)                       # state 1 depends on no parameter


@pytest.mark.parametrize("n_state", [2, 3])
@pytest.mark.parametrize("k", range(len(ac.CPEP_SHAPES)), ids=CPEP_IDS)
def test_cpep_fixed_step_curvature(k, n_state):
    _fixed("cpep", k, n_state)


@pytest.mark.parametrize("k", range(len(ac.SUPP_SHAPES)), ids=SUPP_IDS)
def test_supp_fixed_step_curvature(k):
    _fixed("supp", k, 3)


@pytest.mark.parametrize("acts", ac.GENERAL_ACTS, ids=ACT_IDS)
@pytest.mark.parametrize("shape", ac.CPEP_GENERAL_SHAPES, ids=str)
def test_cpep_fixed_step_curvature_general_activations(shape, acts):
    _fixed("cpep", ac.CPEP_SHAPES.index(shape), 2, acts)


@pytest.mark.parametrize("acts", ac.GENERAL_ACTS, ids=ACT_IDS)
@pytest.mark.parametrize("shape", ac.SUPP_GENERAL_SHAPES, ids=str)
def test_supp_fixed_step_curvature_general_activations(shape, acts):
    _fixed("supp", ac.SUPP_SHAPES.index(shape), 3, acts)


# ----------------------------------------------------------------------------- adaptive
def _adaptive(model, k):
    import curvature_ref as cr
    if model == "cpep":
        arch = ac.CPEP_SHAPES[k]
        c = ac.cpep_case(arch, k, ac.TP6, ac.cpep_subjects(arch))
        N = c["beta"].size
    else:
        c, _, _ = ac.tangent_case("supp", k)
        N = c["theta"].size
    eng = _engine(model, c, 0, 2 if model == "cpep" else 3)
    fwd = eng.forward(want_sse=True)
    sens_out = eng.sensitivity(want_sens=False)
    want = [eng.adaptive_steps(i) for i in range(N)]
    out = eng.curvature()
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
        ref = cr.cpep_curv_replay(c["nn"], c["beta"], ac.cpep_population(c), c["arch"], steps)
    else:
        ref = cr.supp_curv_replay(c["nn"], c["theta"], c["data"], c["tp"], c["arch"], steps)
        assert np.all(out["sens2"][0] == 0.0)
    _check(f"adaptive {model} {c['arch']} N {N}", out, sens_out, ref, ADAPT_RTOL, replay=True)


@pytest.mark.parametrize("k", range(len(ac.CPEP_SHAPES)), ids=CPEP_IDS)
def test_cpep_adaptive_curvature_six_knots(k):
    _adaptive("cpep", k)


@pytest.mark.parametrize("k", range(len(ac.SUPP_SHAPES)), ids=SUPP_IDS)
def test_supp_adaptive_curvature(k):
    _adaptive("supp", k)
