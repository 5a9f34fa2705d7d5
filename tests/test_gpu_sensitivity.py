"""cude_sensitivity on the device (csrc/cude_sens.hip, the tangent policies of csrc/cude_adaptive.h): per-subject output
sensitivities d u / d cond_i, the information sum, the score and the SSE, against

  * the oracle's forward solves in complex arithmetic (tests/sensitivity_ref.py; checked against autograd on the CPU by
    tests/test_sensitivity_host.py) -- in adaptive mode over the device's own accepted steps;
  * the library's own reverse-mode adjoint: g_cond = 2 score / N (independent of the oracle);
  * second differences of cude_forward's per-subject SSE (curvature = 2 info at a noise-free optimum).

Tolerances are the project's: 1e-9 of the reference array's max-norm (GRAD_RTOL, tests/test_gpu_parity.py), 1e-10
relative for SSE, 1e-8 of the max-norm in adaptive mode (tests/test_gpu_adaptive_grad.py).

cude_adaptive_steps reads the gradient's tape, which a plain cude_forward does not write (it returns CUDE_ERR_STATE behind
one); the step sequences after cude_sensitivity are therefore compared with those after cude_loss_grad, whose forward
sweep is cude_forward's solve, and the SSE -- a function of every accepted step -- with cude_forward's own."""
import warnings

import numpy as np
import pytest

from conftest import make_cpep_case, make_supp_case

pytestmark = pytest.mark.gpu

GRAD_RTOL = 1e-9
SSE_RTOL = 1e-10
ADAPT_RTOL = 1e-8


def _pop(c):
    import cude_oracle as o
    return o.CPepPopulation(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"], covariate=(c["arch"][0] == 3))


def _cpep_engine(c, n_steps, n_state=2, model="cpep", cond_space="log", acts=None):
    from cude.engine import Engine
    eng = Engine(model, c["arch"] if model == "cpep" else (1, 0, 0), n_steps=n_steps, n_state=n_state, cond_space=cond_space)
    if acts is not None:
        eng.set_option("hidden_activation", acts[0])
        eng.set_option("output_activation", acts[1])
    eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
    return eng


def _supp_engine(c, n_steps):
    from cude.engine import Engine
    eng = Engine("supp", c["arch"], n_steps=n_steps)
    eng.set_population_supp(c["tp"], c["data"])
    eng.set_params(c["nn"], c["theta"])
    return eng


def _close(name, got, want, rtol):
    scale = np.max(np.abs(want))
    err = np.max(np.abs(got - want))
    print(f"{name}: max err {err:.3e}, max-norm {scale:.3e}, ratio {err / scale if scale else 0.0:.2e}")
    assert err <= rtol * scale, (name, err, scale)


def _check_all(out, ref, rtol, replay=False):
    """replay: the reference replays the device's adaptive steps.  There the per-subject SSEs are held to 1e-10 of their
    largest, the form tests/test_gpu_activations.py uses for SSE arrays (test_gpu_adaptive_grad.py holds their sum to
    1e-10): t_n is a running sum on the device and a tape entry in the replay, a 1e-16 difference in a network input that
    a subject with a small SSE (residuals of 1e-2 on values of order 1) sees amplified by value / residual.  Against
    cude_forward, which takes the same steps in the same arithmetic, the bar is 1e-14 per subject (the callers)."""
    sens, info, score, sse = ref
    _close("sens", out["sens"], sens, rtol)
    _close("info", out["info"], info, rtol)
    _close("score", out["score"], score, rtol)
    print(f"sse: max rel err {np.max(np.abs(out['sse'] - sse) / sse):.3e}, of the largest {np.max(np.abs(out['sse'] - sse)) / np.max(sse):.3e}")
    if replay:
        assert np.max(np.abs(out["sse"] - sse)) <= SSE_RTOL * np.max(sse)
    else:
        assert np.all(np.abs(out["sse"] - sse) <= SSE_RTOL * sse)
    assert np.all(out["sens"][:, 0, :] == 0.0)                      # column t_0 is exactly 0


# ----------------------------------------------------------------------------- 1. fixed-step c-peptide
@pytest.mark.parametrize("N", [200, 57])
@pytest.mark.parametrize("arch,n_state,acts", [((2, 6, 2), 2, None), ((2, 6, 2), 3, None), ((2, 4, 2), 2, None),
                                               ((2, 8, 1), 2, None), ((2, 5, 3), 2, None), ((3, 6, 2), 2, None),
                                               ((2, 4, 2), 2, ("sigmoid", "softplus"))])
def test_cpep_fixed(arch, n_state, acts, N):
    import sensitivity_ref as ref
    c = make_cpep_case(N, arch)
    eng = _cpep_engine(c, 30, n_state, acts=acts)
    eng.set_params(c["nn"], c["beta"])
    out = eng.sensitivity()
    assert out["sens"].shape == (n_state, len(c["tp"]), N)
    _check_all(out, ref.cpep_sens(c["nn"], c["beta"], _pop(c), arch + (acts or ()), 30, n_state), GRAD_RTOL)
    fwd = eng.forward(want_sse=True)
    assert np.all(np.abs(out["sse"] - fwd["sse"]) <= SSE_RTOL * fwd["sse"])
    eng.close()


@pytest.mark.parametrize("N", [200, 57])
@pytest.mark.parametrize("space", ["log", "raw"])
def test_symbolic_fixed(space, N):
    import sensitivity_ref as ref
    c = make_cpep_case(N, (2, 4, 2))
    c["arch"] = (1, 0, 0)
    k = np.exp(c["beta"]) * 20.0 if space == "raw" else c["beta"] + 3.0       # k of the order of the glucose increments
    eng = _cpep_engine(c, 32, model="cpep_sym", cond_space=space)
    eng.set_params([1.78], k)
    out = eng.sensitivity()
    _check_all(out, ref.cpep_sens([1.78], k, _pop(c), (1, 0, 0), 32, 2, space), GRAD_RTOL)
    eng.close()


# ----------------------------------------------------------------------------- 2. fixed-step suppression
@pytest.mark.parametrize("N", [200, 57])
@pytest.mark.parametrize("arch", [(4, 3, 5), (4, 6, 2)])
def test_supp_fixed(arch, N):
    import sensitivity_ref as ref
    c = make_supp_case(N, arch)
    eng = _supp_engine(c, 30)
    out = eng.sensitivity()
    assert np.all(out["sens"][0] == 0.0)                            # state 1 depends on no parameter
    _check_all(out, ref.supp_sens(c["nn"], c["theta"], c["data"], c["tp"], arch, 30), GRAD_RTOL)
    fwd = eng.forward(want_sse=True)
    assert np.all(np.abs(out["sse"] - fwd["sse"]) <= SSE_RTOL * fwd["sse"])
    eng.close()


# ----------------------------------------------------------------------------- 3. the existing adjoint
@pytest.mark.parametrize("n_steps", [30, 0], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("model", ["cpep", "supp"])
def test_score_is_half_the_adjoint_gradient(model, n_steps):
    N = 200
    if model == "cpep":
        c = make_cpep_case(N, (2, 6, 2))
        eng = _cpep_engine(c, n_steps)
        eng.set_params(c["nn"], c["beta"])
    else:
        c = make_supp_case(N)
        eng = _supp_engine(c, n_steps)
    _, _, g_cond = eng.loss_grad()
    out = eng.sensitivity(want_sens=False)
    _close("2 score / N", 2.0 * out["score"] / N, g_cond, GRAD_RTOL)
    eng.close()


# ----------------------------------------------------------------------------- 4. adaptive mode
def _steps(eng, N):
    return [eng.adaptive_steps(i) for i in range(N)]


@pytest.mark.parametrize("arch,N", [((2, 4, 2), 70), ((2, 6, 2), 131), ((3, 4, 2), 64)])
def test_cpep_adaptive(arch, N):
    import sensitivity_ref as ref
    c = make_cpep_case(N, arch)
    eng = _cpep_engine(c, 0)
    eng.set_params(c["nn"], c["beta"])
    eng.loss_grad()
    want = _steps(eng, N)
    fwd = eng.forward(want_sse=True)
    out = eng.sensitivity()
    got = _steps(eng, N)
    for (t0, d0), (t1, d1) in zip(want, got):                       # the accepted steps, bit for bit
        assert np.array_equal(t0, t1) and np.array_equal(d0, d1)
    print(f"sse vs cude_forward: {np.max(np.abs(out['sse'] - fwd['sse']) / fwd['sse']):.3e}")
    assert np.all(np.abs(out["sse"] - fwd["sse"]) <= 1e-14 * fwd["sse"])
    r = ref.cpep_sens_replay(c["nn"], c["beta"], _pop(c), arch, [list(zip(t, dt)) for t, dt in got])
    _check_all(out, r, ADAPT_RTOL, replay=True)
    eng.close()


@pytest.mark.parametrize("space", ["log", "raw"])
def test_symbolic_adaptive(space):
    import sensitivity_ref as ref
    N = 40
    c = make_cpep_case(N, (2, 4, 2))
    c["arch"] = (1, 0, 0)
    k = np.exp(c["beta"]) * 20.0 if space == "raw" else c["beta"] + 3.0
    eng = _cpep_engine(c, 0, model="cpep_sym", cond_space=space)
    eng.set_params([1.78], k)
    out = eng.sensitivity()
    got = _steps(eng, N)
    r = ref.cpep_sens_replay([1.78], k, _pop(c), (1, 0, 0), [list(zip(t, dt)) for t, dt in got], space)
    _check_all(out, r, ADAPT_RTOL, replay=True)
    eng.close()


@pytest.mark.parametrize("arch,N", [((4, 3, 5), 70), ((4, 4, 2), 40)])
def test_supp_adaptive(arch, N):
    import sensitivity_ref as ref
    c = make_supp_case(N, arch)
    eng = _supp_engine(c, 0)
    eng.loss_grad()
    want = _steps(eng, N)
    fwd = eng.forward(want_sse=True)
    out = eng.sensitivity()
    got = _steps(eng, N)
    for (t0, d0), (t1, d1) in zip(want, got):
        assert np.array_equal(t0, t1) and np.array_equal(d0, d1)
    print(f"sse vs cude_forward: {np.max(np.abs(out['sse'] - fwd['sse']) / fwd['sse']):.3e}")
    assert np.all(np.abs(out["sse"] - fwd["sse"]) <= 1e-14 * fwd["sse"])
    r = ref.supp_sens_replay(c["nn"], c["theta"], c["data"], c["tp"], arch, [list(zip(t, dt)) for t, dt in got])
    _check_all(out, r, ADAPT_RTOL, replay=True)
    eng.close()


# ----------------------------------------------------------------------------- 5. curvature
def test_information_is_half_the_curvature_of_the_sse_at_a_noise_free_optimum():
    """Observations generated without noise at the true beta: the residuals vanish there, so d^2 SSE_i / d beta^2 =
    2 info_i exactly, and the central second difference of cude_forward's SSE at beta +- 1e-4 differs from it by the
    h^2 truncation term alone (the oracle by itself: 5.6e-9 of max(2 info))."""
    import cude_oracle as o
    N, arch, h = 200, (2, 6, 2), 1e-4
    c = make_cpep_case(N, arch, noise=0.0)
    _, _, _, _, _, beta_true, _ = o.synthetic_cpep_population(N, 20250905)
    eng = _cpep_engine(c, 30)
    eng.set_params(c["nn"], beta_true)
    out = eng.sensitivity(want_sens=False)
    s0 = eng.forward(want_sse=True)["sse"]
    eng.set_params(None, beta_true + h)
    sp = eng.forward(want_sse=True)["sse"]
    eng.set_params(None, beta_true - h)
    sm = eng.forward(want_sse=True)["sse"]
    curv = (sp - 2.0 * s0 + sm) / h ** 2
    err = np.max(np.abs(curv - 2.0 * out["info"]))
    print(f"curvature: max err {err:.3e} of {np.max(2.0 * out['info']):.3e}: {err / np.max(2.0 * out['info']):.2e}")
    assert err <= 1e-7 * np.max(2.0 * out["info"])
    eng.close()


# ----------------------------------------------------------------------------- 6. edge cases
def test_constant_glucose_is_not_identifiable():
    from cude import api
    N, arch = 70, (2, 6, 2)
    c = make_cpep_case(N, arch)
    c["G"] = c["G"].copy()
    c["G"][[3, 64]] = c["G"][[3, 64], :1]                           # constant glucose: the production never moves
    eng = _cpep_engine(c, 30)
    eng.set_params(c["nn"], c["beta"])
    out = eng.sensitivity()
    assert np.all(out["sens"][:, :, [3, 64]] == 0.0) and np.all(out["info"][[3, 64]] == 0.0)
    flat = out["info"] == 0.0               # (the synthetic population has subjects of its own whose glucose never rises)
    assert np.count_nonzero(~flat) >= N // 2
    eng.close()
    net = api.chain(6, 2, input_dims=2)
    models = [api.CPeptideConditionalUDEModel(c["G"][i], c["tp"], c["age"][i], net, c["obs"][i], bool(c["t2dm"][i]))
              for i in range(N)]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        se = api.conditional_standard_errors(c["beta"], c["nn"], models, c["tp"], c["obs"], n_steps=30)
        ci = api.wald_confidence_intervals(c["beta"], c["nn"], models, c["tp"], c["obs"], n_steps=30)
    assert se[3] == np.inf and se[64] == np.inf and np.array_equal(np.isinf(se), flat) and not np.any(np.isnan(se))
    assert ci[3] == (-np.inf, np.inf)
    api.clear_cache()


@pytest.mark.parametrize("n_steps", [30, 0], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("model", ["cpep", "supp"])
def test_a_failed_subject_is_nan_and_leaves_the_others_alone(model, n_steps):
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
    good = eng.sensitivity()
    assert eng.n_failed() == 0
    bad_cond = cond.copy()
    bad_cond[70] = np.nan
    eng.set_params(nn, bad_cond)
    out = eng.sensitivity()
    assert eng.n_failed() == 1
    assert np.all(np.isnan(out["sens"][:, :, 70])) and all(np.isnan(out[k][70]) for k in ("info", "score", "sse"))
    keep = np.arange(N) != 70
    for k in ("info", "score", "sse"):
        assert np.array_equal(out[k][keep], good[k][keep]), k      # bit for bit
    assert np.array_equal(out["sens"][:, :, keep], good["sens"][:, :, keep])
    # a non-finite network parameter fails every subject
    bad_nn = np.array(nn, dtype=np.float64)
    bad_nn[5] = np.nan
    eng.set_params(bad_nn, cond)
    out = eng.sensitivity()
    assert eng.n_failed() == N
    assert all(np.all(np.isnan(out[k])) for k in ("sens", "info", "score", "sse"))
    eng.close()


def test_the_fallback_kernel_is_reported_as_unsupported():
    from cude._lib import CudeError
    from cude.engine import Engine
    c = make_cpep_case(20, (2, 4, 2))
    eng = Engine("cpep", (2, [5, 9], ["tanh", "relu"], "softplus"), n_steps=30)
    assert eng.fallback_kernel
    eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
    rng = np.random.default_rng(1)
    eng.set_params(0.3 * rng.standard_normal(eng.P), c["beta"])
    with pytest.raises(CudeError) as e:
        eng.sensitivity()
    assert e.value.status == -4 and "fallback kernel" in str(e.value)               # CUDE_ERR_UNSUPPORTED
    assert np.isfinite(eng.forward()["loss"])                                       # the context is still usable
    eng.close()


def test_optional_outputs_and_call_order():
    import ctypes as C
    from cude import _lib
    from cude.engine import Engine
    c = make_cpep_case(57, (2, 4, 2))
    eng = Engine("cpep", (2, 4, 2), n_steps=30)
    lib = _lib.load()
    assert lib.cude_sensitivity(eng._h, None, None, None, None) == -3               # CUDE_ERR_STATE: no population
    eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
    assert lib.cude_sensitivity(eng._h, None, None, None, None) == -3               # no parameters
    eng.set_params(c["nn"], c["beta"])
    full = eng.sensitivity()
    assert lib.cude_sensitivity(eng._h, None, None, None, None) == 0                # all four are optional
    info = np.empty(57)
    assert lib.cude_sensitivity(eng._h, None, info.ctypes.data_as(C.c_void_p), None, None) == 0
    assert np.array_equal(info, full["info"])
    eng.close()


# ----------------------------------------------------------------------------- 7. scale
@pytest.mark.parametrize("model", ["cpep", "supp"])
def test_full_size(model):
    import sensitivity_ref as ref
    N, M = 100000, 400
    if model == "cpep":
        arch = (2, 6, 2)
        c = make_cpep_case(N, arch)
        eng = _cpep_engine(c, 30)
        eng.set_params(c["nn"], c["beta"])
    else:
        arch = (4, 3, 5)
        c = make_supp_case(N, arch)
        eng = _supp_engine(c, 30)
    out = eng.sensitivity()
    failed = eng.n_failed()
    ok = np.isfinite(out["sse"])
    assert np.count_nonzero(~ok) == failed
    assert all(np.all(np.isfinite(out[k][ok])) for k in ("info", "score")) and np.all(np.isfinite(out["sens"][:, :, ok]))
    loss, _, g_cond = eng.loss_grad()
    if failed == 0:
        _close("2 score / N", 2.0 * out["score"] / N, g_cond, GRAD_RTOL)
    idx = np.unique(np.concatenate([np.arange(0, N, N // (M - 10))[:M - 10], np.arange(N - 10, N)]))
    if model == "cpep":
        import cude_oracle as o
        sub = o.CPepPopulation(c["tp"], c["G"][idx], c["obs"][idx], c["age"][idx], c["t2dm"][idx])
        r = ref.cpep_sens(c["nn"], c["beta"][idx], sub, arch, 30)
        _close("sens", out["sens"][:, :, idx], r[0], GRAD_RTOL)
        _close("info", out["info"][idx], r[1], GRAD_RTOL)
        _close("score", out["score"][idx], r[2], GRAD_RTOL)
    else:
        # the scale of the loss's weights is a property of the WHOLE population: the subset is held to the sensitivities
        # themselves and to info / score re-weighted from them
        import cude_oracle as o
        sub = np.ascontiguousarray(c["data"][:, :, idx])
        r = ref.supp_sens(c["nn"], c["theta"][idx], sub, c["tp"], arch, 30)
        _close("sens", out["sens"][:, :, idx], r[0], GRAD_RTOL)
        w2 = (1.0 / o.supp_scale(c["data"]) ** 2)[:, None, None]
        _close("info", out["info"][idx], (w2 * r[0] ** 2).sum(axis=(0, 1)), GRAD_RTOL)
    eng.close()


# ----------------------------------------------------------------------------- 8. mirrors
def test_api_goes_through_the_library(fixed_step_default):
    from cude import api
    N, arch = 57, (2, 6, 2)
    c = make_cpep_case(N, arch)
    eng = _cpep_engine(c, api.fixed_steps(c["tp"]))
    eng.set_params(c["nn"], c["beta"])
    raw = eng.sensitivity()
    eng.close()
    net = api.chain(6, 2, input_dims=2)
    models = [api.CPeptideConditionalUDEModel(c["G"][i], c["tp"], c["age"][i], net, c["obs"][i], bool(c["t2dm"][i]))
              for i in range(N)]
    theta = api.ComponentArray(neural=c["nn"], conditional=c["beta"])
    sens, info, score, sse = api.sensitivities(theta, (models, c["tp"], c["obs"]))
    assert np.array_equal(sens, raw["sens"]) and np.array_equal(info, raw["info"])
    assert np.array_equal(score, raw["score"]) and np.array_equal(sse, raw["sse"])
    ci = api.wald_confidence_intervals(c["beta"], c["nn"], models, c["tp"], c["obs"])
    se = np.sqrt(raw["sse"] / len(c["tp"])) / np.sqrt(raw["info"])
    ok = raw["info"] > 0
    lo, hi = np.array([p[0] for p in ci]), np.array([p[1] for p in ci])
    assert np.allclose((hi - lo)[ok], 2 * 1.959963984540054 * se[ok], rtol=1e-13)
    assert np.allclose(((hi + lo) / 2)[ok], c["beta"][ok], rtol=1e-12, atol=1e-12)
    api.clear_cache()


def test_suppression_api_goes_through_the_library(fixed_step_default):
    from cude import api
    c = make_supp_case(57)
    eng = _supp_engine(c, 30)
    raw = eng.sensitivity()
    eng.close()
    prob = api.SuppressionProblem(api.chain(3, 5, input_dims=4))
    p = api.ComponentArray(theta=c["theta"], neural=c["nn"])
    sens, info, score, sse = api.suppression_sensitivities(p, (prob, c["data"], c["tp"], 0.0))
    assert np.array_equal(sens, raw["sens"]) and np.array_equal(info, raw["info"])
    assert np.array_equal(score, raw["score"]) and np.array_equal(sse, raw["sse"])
    api.clear_cache()
