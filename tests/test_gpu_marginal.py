"""cude_marginal_likelihood on the device against its rules (include/cude.h) restated in mpmath (tests/marginal_ref.py),
driven by the device's OWN numbers: the points it placed (points_out) and their SSEs from
eng.evaluate_conditional_sets(points_out, want_sse=True).

Exact (bitwise): the points against numpy's center + scale * z, in draw mode with z = eng.rng_draws(first_step, K)[0]; the
Metropolis stream around a call; every output for every "profile_chunk"; the subjects beside a failed one.

Bars against the restatement (B = 2^-50 (K + max_k |t_ik| + |log scale_i| + 8): a handful of roundings at magnitude |t| go
into each term, K rounded adds into S0, exp / log accurate to an ulp, a factor of 4 in hand):
  logml      B
  terms      B (the same roundings, one term alone)
  post_mean  B scale max|z|
  post_var   2 B scale^2 S2/S0 -- relative to the SECOND MOMENT, not to the variance (the subtraction cancels): the weights
             carry relative errors of B/4 at most, so S2/S0 moves by 2 B/4 of itself and (S1/S0)^2 <= S2/S0 by 4 B/4: 1.5 B in
             all, rounded up to 2 B
  post_sse   B relative (a weighted mean of positive numbers: twice the weights' relative error)
  ess        2^-50 K relative
  n_bad      exact
sigma: each case's own maximum-likelihood noise level sqrt(median_i SSE_i / T) at the context's parameters -- where a fitted
model's sigma lies, and where the terms near the mode are O(10).  The ess bar carries no |t|: ess depends on differences of
terms, each rounded at its own magnitude, so at K = 2 (sensitivity of ess to t_1 - t_0 up to 0.3) it can only hold for terms
of that size.  Measured with sigma = 1 instead (the suppression and the symbolic case then have SSE/2 = 40 ... 115 at the
centres): ess at K = 2 draws came out at 1.02 ... 1.40 of its bar in those two cases, every other figure at <= 0.55 of its own.

Shapes: N = 70 (one full wave and six lanes) and N = 5; K = 1, 2, 33 and 130; every model, fixed-step and adaptive mode,
the fallback kernel.  Centres and scales are random per subject.

Not reachable from outside: CUDE_ERR_STATE under stream capture (the library captures inside cude_adam_run only, which
calls none of the entry points that batch solves)."""
import math

import numpy as np
import pytest
import torch  # noqa: F401  (first: shared HIP runtime)

import marginal_ref as mr
import test_gpu_predictive as tgp

pytestmark = pytest.mark.gpu

KS = (1, 2, 33, 130)
B50 = 2.0 ** -50
# name -> (prior mean, prior sd, width of the centres' and scales' spread in the case's parameter space)
PRIOR = {"cpep-2441": (-0.6, 0.9, 1.0), "cpep-2661": (-0.6, 0.9, 1.0), "supp-4355": (0.0, 1.0, 1.0), "sym-raw": (20.0, 5.0, 4.0)}
ALL = [(n, False) for n in tgp.CASES] + [("cpep-2441", True)]
ALL_IDS = [n + ("-fallback" if f else "") for n, f in ALL]
RATIOS = {}
SIGMA = 1.0             # (set per case by _setup)
HUGE_NODE = 1e5         # x = center + scale * HUGE_NODE >= 5000: exp(theta) overflows


def _setup(name, n_steps, N, fallback=False):
    """(engine, conditional parameters, centres, scales, prior mean, prior sd); sets SIGMA for the case"""
    global SIGMA
    eng, cond, _ = tgp._make(name, n_steps, N, fallback)
    SIGMA = float(np.sqrt(np.median(eng.forward(want_sse=True)["sse"]) / eng.T))
    pm, sd, spread = PRIOR[name]
    rng = np.random.default_rng(7)
    center = cond + 0.1 * spread * rng.standard_normal(N)
    scale = spread * (0.05 + 0.3 * rng.random(N))
    return eng, cond, center, scale, pm, sd


def _rule(K):
    from cude import api
    return api.gauss_hermite_rule(K)


def _call(eng, source, K, pm, sd, center, scale, **kw):
    if source == "rule":
        z, a = _rule(K)
        return eng.marginal_likelihood(SIGMA, pm, sd, nodes=z, log_weights=a, center=center, scale=scale, want_points=True,
                                       want_terms=True, **kw)
    return eng.marginal_likelihood(SIGMA, pm, sd, n_draws=K, center=center, scale=scale, want_points=True, want_terms=True, **kw)


def _same(tag, got, want, subjects=None):
    for k in ("logml", "post_mean", "post_var", "post_sse", "ess", "n_bad", "points", "terms"):
        g, w = (got[k], want[k]) if subjects is None else (got[k][..., subjects], want[k][..., subjects])
        assert np.array_equal(g, w, equal_nan=True), (tag, k)


def _against_restatement(tag, eng, got, z, a, center, scale, pm, sd):
    """every output of one call against marginal_ref on the device's own points and SSEs; returns the largest error / bar"""
    K = got["points"].shape[0]
    sse = eng.evaluate_conditional_sets(got["points"], want_sse=True)["sse"]
    want = mr.marginal(z, a, got["points"], sse, center, scale, eng.T, SIGMA, pm, sd)
    assert np.array_equal(got["n_bad"], want["n_bad"]), tag
    ok = want["n_bad"] < K
    assert np.all(got["logml"][~ok] == -np.inf)
    for k in ("post_mean", "post_var", "post_sse", "ess"):
        assert np.isnan(got[k][~ok]).all() and np.isfinite(got[k][ok]).all(), (tag, k)
    B = B50 * (K + want["tmax"] + np.abs(np.log(np.where(ok, scale, 1.0))) + 8)
    bars = {"logml": B, "post_mean": B * scale * want["zmax"], "post_var": 2 * B * want["second"],
            "post_sse": B * np.abs(want["post_sse"]), "ess": B50 * K * want["ess"]}
    worst = 0.0
    for k, bar in bars.items():
        err = np.abs(got[k][ok] - want[k][ok])            # (K = 1: z = 0, the bars of both moments are 0 and so is the error)
        ratio = np.max(np.where(err > 0.0, err / np.maximum(bar[ok], 1e-300), 0.0)) if ok.any() else 0.0
        RATIOS[k] = max(RATIOS.get(k, 0.0), float(ratio))
        worst = max(worst, float(ratio))
        assert ratio <= 1.0, (tag, k, ratio)
    good = np.isfinite(want["terms"])
    assert np.array_equal(np.isfinite(got["terms"]), good) and np.all(got["terms"][~good] == -np.inf), tag
    tb = B50 * (np.abs(want["terms"]) + 8)
    tr = np.max(np.abs(got["terms"][good] - want["terms"][good]) / tb[good]) if good.any() else 0.0
    RATIOS["terms"] = max(RATIOS.get("terms", 0.0), float(tr))
    print(f"{tag} sigma={SIGMA:.4g}: error / bar, largest so far: " + ", ".join(f"{k} {v:.3f}" for k, v in RATIOS.items()))
    assert tr <= 1.0, (tag, tr)
    return max(worst, float(tr))


@pytest.mark.parametrize("N", [70, 5])
@pytest.mark.parametrize("n_steps", [30, 0], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("name,fallback", ALL, ids=ALL_IDS)
def test_outputs_match_the_restatement(name, fallback, n_steps, N):
    eng, cond, center, scale, pm, sd = _setup(name, n_steps, N, fallback)
    for K in KS:
        z, a = _rule(K)
        got = _call(eng, "rule", K, pm, sd, center, scale)
        assert np.array_equal(got["points"], center[None, :] + scale[None, :] * z[:, None])
        _against_restatement(f"{name} S={n_steps} N={N} K={K} rule", eng, got, z, a, center, scale, pm, sd)
        assert eng.n_failed() == 0
        for first in (0, 1000):
            normals = eng.rng_draws(first, K)[0]
            got = _call(eng, "draws", K, pm, sd, center, scale, first_step=first)
            assert np.array_equal(got["points"], center[None, :] + scale[None, :] * normals), (K, first)
        _against_restatement(f"{name} S={n_steps} N={N} K={K} draws", eng, got, normals, None, center, scale, pm, sd)
    assert np.array_equal(eng.get_params()[1], cond)            # the context's parameters are untouched
    if n_steps == 0:
        from cude._lib import CudeError
        with pytest.raises(CudeError):
            eng.adaptive_steps(0)
    eng.close()


def test_defaults_for_center_and_scale():
    """center = None: the context's conditional parameters; scale = None: 1"""
    eng, cond, center, scale, pm, sd = _setup("cpep-2441", 30, 70)
    z, a = _rule(33)
    want = eng.marginal_likelihood(SIGMA, pm, sd, nodes=z, log_weights=a, center=cond, scale=np.ones(70), want_points=True,
                                   want_terms=True)
    got = eng.marginal_likelihood(SIGMA, pm, sd, nodes=z, log_weights=a, want_points=True, want_terms=True)
    _same("defaults", got, want)
    flat = eng.marginal_likelihood(SIGMA, 0.3, np.inf, nodes=z, log_weights=a, center=center, scale=scale, want_points=True,
                                   want_terms=True)
    _against_restatement("no prior term", eng, flat, z, a, center, scale, 0.3, np.inf)
    eng.close()


@pytest.mark.parametrize("n_steps", [30, 0], ids=["fixed", "adaptive"])
def test_metropolis_stream_is_undisturbed(n_steps):
    eng, cond, center, scale, pm, sd = _setup("cpep-2441", n_steps, 70)
    chain = lambda: eng.mh_chain(None, None, 0.4, pm, sd, 0.3, n_mc=4)[1]
    eng.set_rng(5)
    plain = np.concatenate([chain(), chain()])
    eng.set_params(None, cond)
    eng.set_rng(5)
    first = chain()
    _call(eng, "draws", 33, pm, sd, center, scale, first_step=2)
    _call(eng, "rule", 2, pm, sd, center, scale)
    assert np.array_equal(np.concatenate([first, chain()]), plain)
    eng.close()


@pytest.mark.parametrize("source", ["rule", "draws"])
@pytest.mark.parametrize("n_steps", [30, 0], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("name", ["cpep-2441", "supp-4355"])
def test_chunks_change_nothing(name, n_steps, source):
    K = 130
    eng, cond, center, scale, pm, sd = _setup(name, n_steps, 70)
    whole = _call(eng, source, K, pm, sd, center, scale)
    for chunk in (1, 7, K):
        eng.set_option("profile_chunk", chunk)
        _same(f"{name} chunk {chunk}", _call(eng, source, K, pm, sd, center, scale), whole)
    eng.close()


@pytest.mark.parametrize("n_steps", [30, 0], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("name", ["supp-4355", "cpep-2441"])
def test_failed_subjects_leave_the_others_alone(name, n_steps):
    K, N = 33, 70
    eng, cond, center, scale, pm, sd = _setup(name, n_steps, N)
    clean = _call(eng, "rule", K, pm, sd, center, scale)
    assert eng.n_failed() == 0 and not clean["n_bad"].any()
    center, scale = center.copy(), scale.copy()
    scale[3], scale[41], center[66] = 0.0, np.nan, np.nan
    failed = np.array([3, 41, 66])
    others = np.setdiff1d(np.arange(N), failed)
    for source in ("rule", "draws"):
        eng.set_option("profile_chunk", 0 if source == "rule" else 8)
        got = _call(eng, source, K, pm, sd, center, scale)
        assert np.all(got["logml"][failed] == -np.inf) and np.all(got["n_bad"][failed] == K) and eng.n_failed() == 3
        for k in ("post_mean", "post_var", "post_sse", "ess"):
            assert np.isnan(got[k][failed]).all(), k
        assert np.all(got["terms"][:, failed] == -np.inf)
        assert not got["n_bad"][others].any()
        if source == "rule":
            _same(name + " beside failed subjects", got, clean, others)
    eng.close()


def test_a_node_with_a_non_finite_sse_is_left_out():
    """Suppression model: theta enters the network as exp(theta), so a node far out drives the solve to a non-finite SSE for
    every subject; it is counted in n_bad and left out of the sums, and the restatement on the device's SSEs agrees."""
    K, N = 5, 70
    eng, cond, center, scale, pm, sd = _setup("supp-4355", 30, N)
    z = np.array([-1.0, 0.0, HUGE_NODE, 0.5, 1.0])
    a = np.array([0.1, 0.2, 0.3, 0.2, 0.1])
    got = eng.marginal_likelihood(SIGMA, pm, np.inf, nodes=z, log_weights=a, center=center, scale=scale, want_points=True,
                                  want_terms=True)
    sse = eng.evaluate_conditional_sets(got["points"], want_sse=True)["sse"]
    bad = ~np.isfinite(sse)
    print("non-finite SSEs per node:", bad.sum(axis=1).tolist())
    assert bad[2].all() and not np.delete(bad, 2, axis=0).any()
    assert np.all(got["n_bad"] == 1) and np.all(got["terms"][2] == -np.inf) and eng.n_failed() == 0
    _against_restatement("non-finite node", eng, got, z, a, center, scale, pm, np.inf)
    keep = [0, 1, 3, 4]
    without = eng.marginal_likelihood(SIGMA, pm, np.inf, nodes=z[keep], log_weights=a[keep], center=center, scale=scale)
    for k in ("logml", "post_mean", "post_var", "post_sse", "ess"):
        assert np.array_equal(got[k], without[k]), k
    eng.close()



def test_argument_and_state_errors():
    from cude._lib import CudeError
    from cude.engine import Engine
    eng, cond, center, scale, pm, sd = _setup("cpep-2441", 30, 5)
    z, a = _rule(5)
    ok = dict(nodes=z, log_weights=a, center=center, scale=scale)
    bad_calls = [
        (lambda: eng.marginal_likelihood(SIGMA, pm, sd, nodes=z, center=center), "both nodes and log_weights"),
        (lambda: eng.marginal_likelihood(SIGMA, pm, sd, log_weights=a, center=center), "both nodes and log_weights"),
        (lambda: eng.marginal_likelihood(SIGMA, pm, sd, **dict(ok, nodes=np.where(np.arange(5) == 2, np.nan, z))), "finite"),
        (lambda: eng.marginal_likelihood(SIGMA, pm, sd, **dict(ok, log_weights=np.where(np.arange(5) == 4, -np.inf, a))), "finite"),
        (lambda: eng.marginal_likelihood(SIGMA, pm, sd, n_draws=4, first_step=-1, center=center), "first_step"),
        (lambda: eng.marginal_likelihood(SIGMA, pm, sd, n_draws=0, center=center), "n_nodes"),
        (lambda: eng.marginal_likelihood(SIGMA, pm, sd, n_draws=65537, center=center), "n_nodes"),
        (lambda: eng.marginal_likelihood(0.0, pm, sd, **ok), "sigma"),
        (lambda: eng.marginal_likelihood(-1.0, pm, sd, **ok), "sigma"),
        (lambda: eng.marginal_likelihood(np.inf, pm, sd, **ok), "sigma"),
        (lambda: eng.marginal_likelihood(np.nan, pm, sd, **ok), "sigma"),
        (lambda: eng.marginal_likelihood(SIGMA, pm, 0.0, **ok), "prior_sd"),
        (lambda: eng.marginal_likelihood(SIGMA, pm, -2.0, **ok), "prior_sd"),
        (lambda: eng.marginal_likelihood(SIGMA, pm, np.nan, **ok), "prior_sd"),
        (lambda: eng.marginal_likelihood(SIGMA, np.inf, sd, **ok), "prior_mean"),
        (lambda: eng.marginal_likelihood(SIGMA, np.nan, sd, **ok), "prior_mean"),
    ]
    for call, word in bad_calls:
        with pytest.raises(CudeError) as e:
            call()
        assert e.value.status == -1 and word in str(e.value), e.value            # CUDE_ERR_ARG
    # no output requested: only the C entry point can be asked for nothing
    from cude._lib import check
    from cude.engine import _ptr
    none = [None] * 8
    with pytest.raises(CudeError) as e:
        check(eng._lib.cude_marginal_likelihood(eng._h, 5, _ptr(z), _ptr(a), 0, _ptr(center), _ptr(scale), SIGMA, pm, sd, *none))
    assert e.value.status == -1 and "no output" in str(e.value)
    # ... and for one output alone
    logml = np.empty(5)
    check(eng._lib.cude_marginal_likelihood(eng._h, 5, _ptr(z), _ptr(a), 0, _ptr(center), _ptr(scale), SIGMA, pm, sd,
                                            _ptr(logml), *none[1:]))
    assert np.array_equal(logml, eng.marginal_likelihood(SIGMA, pm, sd, **ok)["logml"])
    eng.close()
    # CUDE_ERR_STATE
    c = tgp._case("cpep", (2, 4, 2), 5)
    eng = Engine("cpep", (2, 4, 2), n_steps=30, n_state=3)
    with pytest.raises(CudeError) as e:
        eng.marginal_likelihood(SIGMA, pm, sd, nodes=z, log_weights=a)
    assert e.value.status == -3 and "population" in str(e.value)
    eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
    with pytest.raises(CudeError) as e:
        eng.marginal_likelihood(SIGMA, pm, sd, **ok)
    assert e.value.status == -3 and "shared parameters" in str(e.value)
    eng.set_params(c["nn"], None)
    with pytest.raises(CudeError) as e:
        eng.marginal_likelihood(SIGMA, pm, sd, nodes=z, log_weights=a)
    assert e.value.status == -3 and "conditional parameters" in str(e.value)
    assert np.isfinite(eng.marginal_likelihood(SIGMA, pm, sd, **ok)["logml"]).all()       # (a centre of the caller's: fine)
    eng.close()


def _e2e_models(api, c):
    net = api.chain(c["arch"][1], c["arch"][2], "tanh")
    return [api.CPeptideConditionalUDEModel(c["G"][i], c["tp"], c["age"][i], net, c["obs"][i], bool(c["t2dm"][i]))
            for i in range(len(c["beta"]))]


def test_end_to_end_quadrature_against_grid():
    """cpep-2441, six subjects, 30 steps, sigma = 0.03, prior Normal(-1, 0.8^2): the 33-node Gauss-Hermite rule at the MAP
    against the trapezoid rule on 4 001 points over mu -/+ 8 Omega, both through api.marginal_likelihood.

    The numpy oracle's own two rules on exactly this case (tests/marginal_ref.py end_to_end_oracle, also held by
    tests/test_marginal_host.py) differ by 1.8e-15, 5.6e-2, 3.9e-14, 9.0e-9, 1.2e-9, 1.4e-14: subject 1 has a second hump
    that a rule centred at the mode does not see and is left out (at most one may be).  Bar for the others: ten times the
    oracle's largest gap among them (9.0e-9) plus 1e-10 / (2 sigma^2) = 5.6e-8 for the device-against-oracle SSE tolerance
    of the parity tests.  Also: Laplace (Q = 1) is further from the grid than Q = 33, and importance sampling with 2 048
    device draws (seed 20250905, for which the oracle-side replay of the draws lies within 1.3 standard errors) lies
    within five of its own standard errors sqrt(1 / ess - 1 / K) of the Q = 33 value."""
    from cude import api
    from conftest import device_draw
    e = mr.E2E
    orc = mr.end_to_end_oracle()
    c, keep = orc["case"], orc["keep"]
    gap = np.abs(orc["q33"] - orc["grid"])
    print("oracle gaps:", gap, "kept:", keep)
    assert np.sum(~keep) <= 1
    bar = 10.0 * np.max(gap[keep]) + 1e-10 / (2.0 * e["sigma"] ** 2)
    # the oracle-side replay of the importance sample for the seed used below
    K, N, T = e["n_draws"], e["N"], len(c["tp"])
    z = np.array([[device_draw(e["seed"], i, k)[0] for i in range(N)] for k in range(K)])
    x = orc["center"][None, :] + orc["scale"][None, :] * z
    rep = mr.marginal_numpy(z, 0.5 * math.log(2 * math.pi) - math.log(K) + 0.5 * z * z, x, mr.oracle_sse(c, x, e["n_steps"]),
                            orc["center"], orc["scale"], T, e["sigma"], e["prior_mean"], e["omega"])
    rep_se = np.sqrt(1.0 / rep["ess"] - 1.0 / K)
    print("oracle replay (IS - Q33) / se:", (rep["logml"] - orc["q33"]) / rep_se)
    assert np.all(np.abs(rep["logml"] - orc["q33"])[keep] <= 5.0 * rep_se[keep])
    models = _e2e_models(api, c)
    args = (None, c["nn"], models, c["tp"], c["obs"], e["sigma"], e["prior_mean"], e["omega"])
    try:
        q33 = api.marginal_likelihood(*args, method="quadrature", n_nodes=33, n_steps=e["n_steps"])
        q1 = api.marginal_likelihood(*args, method="quadrature", n_nodes=1, n_steps=e["n_steps"])
        grid = api.marginal_likelihood(*args, method="grid", n_nodes=e["n_grid"], grid_halfwidth=e["halfwidth"],
                                       n_steps=e["n_steps"])
        imp = api.marginal_likelihood(*args, method="importance", n_nodes=K, seed=e["seed"], n_steps=e["n_steps"])
    finally:
        api.clear_cache()
    print("device Q33 - grid:", q33.logml - grid.logml, " bar", bar)
    print("device grid - oracle grid:", grid.logml - orc["grid"], " Q33:", q33.logml - orc["q33"])
    assert np.all(np.abs(q33.logml - grid.logml)[keep] <= bar)
    assert np.all(np.abs(q1.logml - grid.logml)[keep] > np.abs(q33.logml - grid.logml)[keep])
    se = np.sqrt(1.0 / imp.ess - 1.0 / K)
    print("device (IS - Q33) / se:", (imp.logml - q33.logml) / se, " ess", imp.ess)
    assert np.all(np.abs(imp.logml - q33.logml)[keep] <= 5.0 * se[keep])
    assert not grid.n_bad.any() and not q33.n_bad.any()


def test_api_mirror_returns_the_engine_numbers():
    from cude import api
    arch, N = (2, 4, 2), 24
    c = tgp._case("cpep", arch, N)
    models = tgp._api_models(api, c, arch, N)
    sigma, pm, om = 0.4, -0.6, 0.9
    try:
        got = api.marginal_likelihood(c["beta"], c["nn"], models, c["tp"], c["obs"], sigma, pm, om, n_nodes=9, n_steps=30)
        norm = api.marginal_likelihood(c["beta"], c["nn"], models, c["tp"], c["obs"], sigma, pm, om, n_nodes=9, n_steps=30,
                                       normalized=True)
        eng = api._population(models, c["tp"], c["obs"], 30).engine
        z, a = api.gauss_hermite_rule(9)
        r = eng.refine_conditional(c["beta"], -6.0, 4.0, penalty_weight=(sigma / om) ** 2, penalty_center=pm)
        assert np.array_equal(got.center, r["x"]) and np.array_equal(got.scale, sigma / np.sqrt(r["info"] + (sigma / om) ** 2))
        want = eng.marginal_likelihood(sigma, pm, om, nodes=z, log_weights=a, center=got.center, scale=got.scale)
        for k in ("logml", "post_mean", "post_var", "post_sse", "ess", "n_bad"):
            assert np.array_equal(getattr(got, k), want[k]), k
        total = 0.0
        for v in got.logml:
            total = total + v
        assert got.total == total
        assert np.array_equal(norm.logml, got.logml - 0.5 * len(c["tp"]) * math.log(2.0 * math.pi))
        s2, mu, om2 = api.em_updates(got.post_mean, got.post_var, got.post_sse, len(c["tp"]))
        assert s2 > 0 and om2 > 0 and abs(mu - np.mean(got.post_mean)) <= 1e-15
    finally:
        api.clear_cache()
