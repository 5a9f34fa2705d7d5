"""cude_curvature on the device beyond the per-shape checks of tests/test_gpu_curvature_shapes.py: the symbolic model in
both cond_spaces, the adaptive step sequence, failures, error codes, what the call leaves alone, and the api layer built
on it (observed standard errors, the Laplace value with the observed scale, map_curvature).

References: tests/curvature_ref.py (route (b); every network here is tanh / softplus or the symbolic model, where the
stencil is valid -- tests/test_curvature_host.py).  Bars: GRAD_RTOL / ADAPT_RTOL / SSE_RTOL of tests/test_gpu_sensitivity.py;
the api checks use the logml bar of tests/test_gpu_marginal.py's end-to-end case.

Not reachable from outside: CUDE_ERR_STATE under stream capture (the library captures inside cude_adam_run only)."""
import ctypes as C
import math

import numpy as np
import pytest

import marginal_ref as mr
from conftest import make_cpep_case, make_supp_case
from test_gpu_sensitivity import ADAPT_RTOL, GRAD_RTOL, SSE_RTOL, _cpep_engine, _pop, _supp_engine

pytestmark = pytest.mark.gpu


def _ratio(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _hold(tag, out, ref, rtol, replay=False):
    r = {k: _ratio(out[k], ref[k]) for k in ("sens2", "curv", "info", "score")}
    top = float(np.max(np.abs(out["sse"] - ref["sse"])) / np.max(ref["sse"]))
    rel = float(np.max(np.abs(out["sse"] - ref["sse"]) / ref["sse"]))
    print(f"{tag}: ratios sens2 {r['sens2']:.2e} curv {r['curv']:.2e} info {r['info']:.2e} score {r['score']:.2e} "
          f"sse {rel:.2e} (of the largest {top:.2e})")
    assert all(v <= rtol for v in r.values()), r
    assert (top if replay else rel) <= SSE_RTOL
    assert np.all(out["sens2"][:, 0, :] == 0.0)


# ----------------------------------------------------------------------------- 1. the symbolic model
def _symbolic(space, N):
    c = make_cpep_case(N, (2, 4, 2))
    c["arch"] = (1, 0, 0)
    k = np.exp(c["beta"]) * 20.0 if space == "raw" else c["beta"] + 3.0       # k of the order of the glucose increments
    return c, k


@pytest.mark.parametrize("n_state", [2, 3])
@pytest.mark.parametrize("space", ["log", "raw"])
def test_symbolic_fixed(space, n_state):
    import curvature_ref as cr
    c, k = _symbolic(space, 70)
    eng = _cpep_engine(c, 32, n_state=n_state, model="cpep_sym", cond_space=space)
    eng.set_params([1.78], k)
    out = eng.curvature()
    assert eng.n_failed() == 0
    eng.close()
    _hold(f"symbolic {space} n_state {n_state}", out, cr.cpep_curv([1.78], k, _pop(c), (1, 0, 0), 32, n_state, space), GRAD_RTOL)


@pytest.mark.parametrize("space", ["log", "raw"])
def test_symbolic_adaptive(space):
    import curvature_ref as cr
    N = 40
    c, k = _symbolic(space, N)
    eng = _cpep_engine(c, 0, model="cpep_sym", cond_space=space)
    eng.set_params([1.78], k)
    out = eng.curvature()
    got = [eng.adaptive_steps(i) for i in range(N)]
    eng.close()
    ref = cr.cpep_curv_replay([1.78], k, _pop(c), (1, 0, 0), [list(zip(t, dt)) for t, dt in got], space)
    _hold(f"symbolic adaptive {space}", out, ref, ADAPT_RTOL, replay=True)


# ----------------------------------------------------------------------------- 2. the adaptive steps are cude_forward's
@pytest.mark.parametrize("model", ["cpep", "supp"])
def test_adaptive_steps_are_the_forward_solves(model):
    N = 70
    if model == "cpep":
        c = make_cpep_case(N, (2, 6, 2))
        eng = _cpep_engine(c, 0)
        eng.set_params(c["nn"], c["beta"])
    else:
        c = make_supp_case(N, (4, 4, 2))
        eng = _supp_engine(c, 0)
    eng.loss_grad()                                                # (its forward sweep is cude_forward's solve)
    want = [eng.adaptive_steps(i) for i in range(N)]
    fwd = eng.forward(want_sse=True)
    out = eng.curvature(want_sens2=False)
    got = [eng.adaptive_steps(i) for i in range(N)]
    eng.close()
    for (t0, d0), (t1, d1) in zip(want, got):
        assert np.array_equal(t0, t1) and np.array_equal(d0, d1)
    assert np.all(np.abs(out["sse"] - fwd["sse"]) <= 1e-14 * fwd["sse"])


# ----------------------------------------------------------------------------- 3. failures
KEYS = ("curv", "info", "score", "sse")


def _failure_case(model, n_steps):
    N = 131
    if model == "cpep":
        c = make_cpep_case(N, (2, 6, 2))
        eng = _cpep_engine(c, n_steps)
        nn, cond = c["nn"], c["beta"]
    else:
        c = make_supp_case(N)
        eng = _supp_engine(c, n_steps)
        nn, cond = c["nn"], c["theta"]
    eng.set_params(nn, cond)
    return eng, np.array(nn, dtype=np.float64), np.array(cond, dtype=np.float64), N


def _only_subject_fails(eng, good, i, N):
    out = eng.curvature()
    assert eng.n_failed() == 1
    assert np.all(np.isnan(out["sens2"][:, :, i])) and all(np.isnan(out[k][i]) for k in KEYS)
    keep = np.arange(N) != i
    for k in KEYS:
        assert np.array_equal(out[k][keep], good[k][keep]), k       # bit for bit
    assert np.array_equal(out["sens2"][:, :, keep], good["sens2"][:, :, keep])


@pytest.mark.parametrize("n_steps", [30, 0], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("model", ["cpep", "supp"])
def test_a_failed_subject_is_nan_and_leaves_the_others_alone(model, n_steps):
    eng, nn, cond, N = _failure_case(model, n_steps)
    good = eng.curvature()
    assert eng.n_failed() == 0 and all(np.all(np.isfinite(good[k])) for k in KEYS + ("sens2",))
    bad = cond.copy()
    bad[70] = np.nan
    eng.set_params(nn, bad)
    _only_subject_fails(eng, good, 70, N)
    if model == "supp":                                            # exp(theta) overflows: a non-finite network input
        bad = cond.copy()
        bad[3] = 5000.0
        eng.set_params(nn, bad)
        _only_subject_fails(eng, good, 3, N)
    bad_nn = nn.copy()
    bad_nn[5] = np.nan                                             # a non-finite network parameter fails every subject
    eng.set_params(bad_nn, cond)
    out = eng.curvature()
    assert eng.n_failed() == N
    assert all(np.all(np.isnan(out[k])) for k in KEYS + ("sens2",))
    eng.close()


# ----------------------------------------------------------------------------- 4. error codes, optional outputs
def test_error_codes_by_their_messages():
    from cude import _lib
    from cude._lib import CudeError
    from cude.engine import Engine
    c = make_cpep_case(57, (2, 4, 2))
    eng = Engine("cpep", (2, 4, 2), n_steps=30)
    with pytest.raises(CudeError) as e:
        eng.curvature()
    assert e.value.status == -3 and "population not set" in str(e.value)           # CUDE_ERR_STATE
    eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
    with pytest.raises(CudeError) as e:
        eng.curvature()
    assert e.value.status == -3 and "parameters not set" in str(e.value)
    eng.set_params(c["nn"], c["beta"])
    lib = _lib.load()
    with pytest.raises(CudeError) as e:
        _lib.check(lib.cude_curvature(eng._h, None, None, None, None, None))
    assert e.value.status == -1 and "no output requested" in str(e.value)           # CUDE_ERR_ARG
    full = eng.curvature()
    curv = np.empty(57)
    assert lib.cude_curvature(eng._h, None, curv.ctypes.data_as(C.c_void_p), None, None, None) == 0
    assert np.array_equal(curv, full["curv"])
    sse = np.empty(57)
    assert lib.cude_curvature(eng._h, None, None, None, None, sse.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(sse, full["sse"])
    eng.close()
    # the fallback kernel
    eng = Engine("cpep", (2, [5, 9], ["tanh", "relu"], "softplus"), n_steps=30)
    assert eng.fallback_kernel
    eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
    eng.set_params(0.3 * np.random.default_rng(1).standard_normal(eng.P), c["beta"])
    with pytest.raises(CudeError) as e:
        eng.curvature()
    assert e.value.status == -4 and "fallback kernel" in str(e.value)               # CUDE_ERR_UNSUPPORTED
    assert np.isfinite(eng.forward()["loss"])                                       # the context is still usable
    eng.close()
    # a general-activation network in adaptive mode: no order-2 kernel
    eng = _cpep_engine(c, 0, acts=("sigmoid", "softplus"))
    eng.set_params(c["nn"], c["beta"])
    with pytest.raises(CudeError) as e:
        eng.curvature()
    assert e.value.status == -4 and "no order-2 kernel" in str(e.value)
    eng.close()


# ----------------------------------------------------------------------------- 5. what the call leaves alone
def test_parameters_and_a_metropolis_chain_are_untouched():
    N, n_mc = 70, 5
    c = make_cpep_case(N, (2, 4, 2))
    rng = np.random.default_rng(5)
    normals, uniforms = rng.standard_normal((n_mc, N)), rng.random((n_mc, N))
    args = (0.3, -1.0, 0.8, 0.2)                                    # sigma, prior mean, prior sd, proposal sd
    eng = _cpep_engine(c, 30)
    eng.set_params(c["nn"], c["beta"])
    _, whole = eng.mh_chain(normals, uniforms, *args)
    eng.set_params(c["nn"], c["beta"])
    _, head = eng.mh_chain(normals[:2], uniforms[:2], *args)
    nn0, cond0 = eng.get_params()
    eng.curvature()
    nn1, cond1 = eng.get_params()
    _, tail = eng.mh_chain(normals[2:], uniforms[2:], *args)
    eng.close()
    assert np.array_equal(nn0, nn1) and np.array_equal(cond0, cond1)
    assert np.array_equal(np.concatenate([head, tail]), whole)


# ----------------------------------------------------------------------------- 6. the api layer
def _e2e_models(api, c):
    net = api.chain(c["arch"][1], c["arch"][2], "tanh")
    return [api.CPeptideConditionalUDEModel(c["G"][i], c["tp"], c["age"][i], net, c["obs"][i], bool(c["t2dm"][i]))
            for i in range(len(c["beta"]))]


def test_api_at_the_maps_of_the_end_to_end_case():
    """cpep-2441, six subjects, 30 steps, sigma = 0.03, prior Normal(-1, 0.8^2) (tests/marginal_ref.py E2E).  At the MAPs
    the device's own refinement returns: map_curvature's classes are the signs of the reference curvature + pw; the
    observed standard errors and the "laplace" values with the observed scale equal their restatements built from the
    reference curvature (tests/curvature_ref.py, the oracle's SSE) within the logml bar of that case; the defaults are the
    calls without the new keywords, bit for bit."""
    import curvature_ref as cr
    from cude import api
    e = mr.E2E
    orc = mr.end_to_end_oracle()
    c, keep = orc["case"], orc["keep"]
    bar = 10.0 * np.max(np.abs(orc["q33"] - orc["grid"])[keep]) + 1e-10 / (2.0 * e["sigma"] ** 2)
    sigma, pm, om, S = e["sigma"], e["prior_mean"], e["omega"], e["n_steps"]
    pw, T = (sigma / om) ** 2, len(c["tp"])
    models = _e2e_models(api, c)
    args = (None, c["nn"], models, c["tp"], c["obs"], sigma, pm, om)
    try:
        lap_obs = api.marginal_likelihood(*args, method="laplace", curvature="observed", n_steps=S)
        lap_exp = api.marginal_likelihood(*args, method="laplace", n_steps=S)
        q1 = api.marginal_likelihood(*args, method="quadrature", n_nodes=1, n_steps=S)
        q1e = api.marginal_likelihood(*args, method="quadrature", n_nodes=1, curvature="expected", n_steps=S)
        q5_obs = api.marginal_likelihood(*args, method="quadrature", n_nodes=5, curvature="observed", n_steps=S)
        x = lap_obs.center
        mc = api.map_curvature(x, c["nn"], models, c["tp"], c["obs"], sigma=sigma, prior_omega=om, n_steps=S)
        se_obs = api.conditional_standard_errors(x, c["nn"], models, c["tp"], c["obs"], sigma=sigma, n_steps=S,
                                                 information="observed")
        se_def = api.conditional_standard_errors(x, c["nn"], models, c["tp"], c["obs"], sigma=sigma, n_steps=S)
        se_exp = api.conditional_standard_errors(x, c["nn"], models, c["tp"], c["obs"], sigma=sigma, n_steps=S,
                                                 information="expected")
        ci_obs = api.wald_confidence_intervals(x, c["nn"], models, c["tp"], c["obs"], sigma=sigma, n_steps=S,
                                               information="observed")
        theta = api.ComponentArray(neural=c["nn"], conditional=x)
        _, info, _, sse = api.sensitivities(theta, (models, c["tp"], c["obs"]), n_steps=S)
        sens2, curv, info2, score2, sse2 = api.curvatures(theta, (models, c["tp"], c["obs"]), n_steps=S)
    finally:
        api.clear_cache()
    # defaults: today's calls, bit for bit
    for k in ("logml", "center", "scale", "post_mean", "post_var"):
        assert np.array_equal(getattr(lap_exp, k), getattr(q1, k)) and np.array_equal(getattr(q1e, k), getattr(q1, k)), k
    assert not hasattr(q1, "curvature_fallback")
    assert np.all(info > 0) and np.array_equal(se_def, se_exp) and np.array_equal(se_def, sigma / np.sqrt(info))
    assert np.array_equal(info2, info) and np.array_equal(sse2, sse) and sens2.shape == (2, T, e["N"])
    # the reference at the device's centres
    ref = cr.cpep_curv(c["nn"], x, _pop(c), c["arch"], S, 2)
    print("curv / info at the MAPs:", ref["curv"] / ref["info"], " curv + pw:", ref["curv"] + pw, " bar", bar)
    print("device curv vs reference:", _ratio(curv, ref["curv"]))
    assert _ratio(curv, ref["curv"]) <= GRAD_RTOL
    a_ref, b_ref, ratio_ref, cls_ref = cr.map_classes(ref["curv"], ref["info"], pw)
    assert np.array_equal(mc.status, cls_ref), (mc.status, cls_ref)
    assert np.all(np.abs(mc.observed - a_ref) <= GRAD_RTOL * np.max(np.abs(a_ref)))
    assert np.all(np.abs(mc.expected - b_ref) <= GRAD_RTOL * np.max(np.abs(b_ref)))
    assert np.allclose(mc.ratio, ratio_ref, rtol=1e-6)
    # observed standard errors against the restatement
    se_ref = cr.observed_se(ref["curv"], sigma)
    print("observed se:", se_obs, " restated:", se_ref, " expected:", se_def)
    assert np.array_equal(np.isinf(se_obs), np.isinf(se_ref))
    fin = np.isfinite(se_ref)
    assert np.all(np.abs(se_obs[fin] - se_ref[fin]) <= bar * se_ref[fin])
    z = 1.959963984540054
    for (lo, hi), b, s in zip(ci_obs, x, se_obs):
        assert (lo, hi) == (-np.inf, np.inf) if np.isinf(s) else abs((hi - lo) - 2 * z * s) <= 1e-12 * s + 1e-15
    # the Laplace value with the observed scale, restated on the oracle's SSE and the reference curvature
    fb = np.zeros(e["N"], dtype=bool)
    fb[lap_obs.curvature_fallback] = True
    assert np.array_equal(fb, ~(ref["curv"] + pw > 0))
    scale_ref = np.where(fb, sigma / np.sqrt(ref["info"] + pw), sigma / np.sqrt(np.where(fb, 1.0, ref["curv"] + pw)))
    z1, a1 = api.gauss_hermite_rule(1)
    want = mr.marginal_numpy(z1, a1, x[None, :], mr.oracle_sse(c, x[None, :], S), x, scale_ref, T, sigma, pm, om)["logml"]
    print("laplace (observed) - restatement:", lap_obs.logml - want)
    print("gaps to the oracle's grid: Q1 expected", q1.logml - orc["grid"], " Q1 observed", lap_obs.logml - orc["grid"],
          " Q5 observed", q5_obs.logml - orc["grid"])
    assert np.all(np.abs(lap_obs.logml - want) <= bar)
    assert np.array_equal(lap_obs.center, q1.center)
    assert np.all(np.abs(lap_obs.scale - scale_ref) <= bar * scale_ref)


def test_api_mirrors_return_the_engine_numbers(fixed_step_default):
    from cude import api
    N, arch = 57, (2, 6, 2)
    c = make_cpep_case(N, arch)
    eng = _cpep_engine(c, api.fixed_steps(c["tp"]))
    eng.set_params(c["nn"], c["beta"])
    raw = eng.curvature()
    eng.close()
    net = api.chain(6, 2, input_dims=2)
    models = [api.CPeptideConditionalUDEModel(c["G"][i], c["tp"], c["age"][i], net, c["obs"][i], bool(c["t2dm"][i]))
              for i in range(N)]
    theta = api.ComponentArray(neural=c["nn"], conditional=c["beta"])
    got = api.curvatures(theta, (models, c["tp"], c["obs"]))
    api.clear_cache()
    for v, k in zip(got, ("sens2", "curv", "info", "score", "sse")):
        assert np.array_equal(v, raw[k]), k
    s = make_supp_case(57)
    eng = _supp_engine(s, 30)
    raw = eng.curvature()
    eng.close()
    prob = api.SuppressionProblem(api.chain(3, 5, input_dims=4))
    p = api.ComponentArray(theta=s["theta"], neural=s["nn"])
    got = api.suppression_curvatures(p, (prob, s["data"], s["tp"], 0.0))
    api.clear_cache()
    for v, k in zip(got, ("sens2", "curv", "info", "score", "sse")):
        assert np.array_equal(v, raw[k]), k
    assert np.all(raw["sens2"][0] == 0.0)
    with pytest.raises(ValueError):
        api.conditional_standard_errors(c["beta"], c["nn"], models, c["tp"], c["obs"], information="exact")
