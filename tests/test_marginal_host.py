"""Host side of the per-subject marginal likelihoods: the declarations of the entry point in every binding, the mpmath
restatement of its rules (tests/marginal_ref.py) against a Gaussian integral in closed form, rule 3's running rescaled
sums in doubles against that restatement, and the mirror's rule builders and helpers."""
import math
import os
import re

import numpy as np
import pytest

import marginal_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B50 = 2.0 ** -50


def test_every_binding_declares_the_entry_point():
    header = open(os.path.join(ROOT, "include", "cude.h")).read()
    julia = open(os.path.join(ROOT, "conditional-ude_amd", "julia", "CUDEHip.jl")).read()
    from cude import _lib, api
    from cude.engine import Engine
    assert re.search(r"int32_t\s+cude_marginal_likelihood\s*\(", header)
    assert "cude_marginal_likelihood" in _lib.exported_symbols()
    assert ":cude_marginal_likelihood," in julia
    assert hasattr(Engine, "marginal_likelihood")
    for name in ("gauss_hermite_rule", "grid_rule", "marginal_likelihood", "information_criteria", "em_updates"):
        assert callable(getattr(api, name)), name
        assert re.search(r"(?m)^function %s\(" % name, julia), name


# SSE(x) = c + h (x - xhat)^2: (c, h, xhat, n_obs, sigma, prior_mean, prior_sd)
GAUSSIAN = [(1.3, 7.0, -0.4, 5, 0.4, -0.6, 0.9), (0.02, 55.0, 0.7, 8, 0.03, -1.0, 0.8), (4.0, 0.5, 2.0, 5, 1.5, 0.0, 3.0)]


@pytest.mark.parametrize("Q", [1, 5, 33])
def test_restatement_reproduces_the_gaussian_integral(Q):
    """Centred at the mode with the exact scale the integrand times exp(z^2 / 2) is a constant, which every Gauss-Hermite
    rule integrates exactly: logml to 1e-12 for Q = 1, 5, 33; the posterior mean is the mode; from Q = 2 on the variance
    and E[SSE] (degree 2 in z) are exact too."""
    from cude import api
    z, a = api.gauss_hermite_rule(Q)
    for c, h, xhat, T, sigma, pm, sd in GAUSSIAN:
        want, m, s, esse = mr.gaussian_case(c, h, xhat, T, sigma, pm, sd)
        center, scale = np.array([float(m)]), np.array([float(s)])
        x = center[None, :] + scale[None, :] * z[:, None]
        sse = c + h * (x - xhat) ** 2
        got = mr.marginal(z, a, x, sse, center, scale, T, sigma, pm, sd)
        print(f"Q={Q} sigma={sigma}: logml {got['logml'][0]:.15g} closed form {float(want):.15g}")
        assert abs(got["logml"][0] - float(want)) <= 1e-12
        assert abs(got["post_mean"][0] - float(m)) <= 1e-12 and got["n_bad"][0] == 0
        if Q == 1:
            assert got["post_var"][0] == 0.0 and got["ess"][0] == 1.0
        else:
            assert abs(got["post_var"][0] - float(s) ** 2) <= 1e-12 * float(s) ** 2
            assert abs(got["post_sse"][0] - float(esse)) <= 1e-11 * float(esse)


def _rule3_doubles(z, a, x, sse, center, scale, T, sigma, pm, sd):
    """Rules 2-4 as the kernels evaluate them, in doubles, for one subject"""
    ll_const, inv = -(T / 2.0) * math.log(sigma * sigma), 1.0 / (2.0 * sigma * sigma)
    M, S0, S1, S2, S3, Qq, bad = -math.inf, 0.0, 0.0, 0.0, 0.0, 0.0, 0
    for k in range(len(z)):
        t = -math.inf
        if math.isfinite(sse[k]):
            u = (x[k] - pm) / sd
            t = (a[k] + (-sse[k] * inv + ll_const)) + ((-0.5 * (u * u) - math.log(sd)) - 0.5 * math.log(2 * math.pi))
        if not math.isfinite(t):
            bad += 1
            continue
        if t > M:
            r = math.exp(M - t)
            S0, S1, S2, S3, Qq, M, e = S0 * r, S1 * r, S2 * r, S3 * r, Qq * (r * r), t, 1.0
        else:
            e = math.exp(t - M)
        S0, S1, S2, S3, Qq = S0 + e, S1 + e * z[k], S2 + e * (z[k] * z[k]), S3 + e * sse[k], Qq + e * e
    if bad == len(z):
        return dict(logml=-math.inf, post_mean=math.nan, post_var=math.nan, post_sse=math.nan, ess=math.nan, n_bad=bad)
    m1, m2 = S1 / S0, S2 / S0
    return dict(logml=(M + math.log(S0)) + math.log(scale), post_mean=center + scale * m1,
                post_var=(scale * scale) * max(0.0, m2 - m1 * m1), post_sse=S3 / S0, ess=(S0 * S0) / Qq, n_bad=bad)


@pytest.mark.parametrize("K", [1, 2, 33, 130])
def test_running_rescaled_sums_match_the_restatement(K):
    """Rule 3 in doubles on a skewed, wavy SSE with terms in increasing and decreasing stretches (both branches of the
    rescaling are taken), a bad node among them: the restatement's values within the bars the GPU tests use
    (tests/test_gpu_marginal.py)."""
    rng = np.random.default_rng(K)
    T, sigma, pm, sd, center, scale = 5, 0.4, -0.6, 0.9, -0.3, 0.21
    z = np.sort(rng.standard_normal(K)) * 2.0
    a = rng.normal(size=K)
    x = center + scale * z
    sse = 1.0 + 3.0 * (x + 0.5) ** 2 * (1.0 + 0.4 * np.sin(5.0 * x)) + 0.3 * np.cos(3.0 * x)
    if K > 2:
        sse[K // 3] = np.inf
    want = mr.marginal(z, a, x[:, None], sse[:, None], [center], [scale], T, sigma, pm, sd)
    got = _rule3_doubles(z, a, x, sse, center, scale, T, sigma, pm, sd)
    bar = B50 * (K + want["tmax"][0] + abs(math.log(scale)) + 8)
    assert got["n_bad"] == want["n_bad"][0] == (1 if K > 2 else 0)
    assert abs(got["logml"] - want["logml"][0]) <= bar
    assert abs(got["post_mean"] - want["post_mean"][0]) <= bar * scale * want["zmax"][0]
    assert abs(got["post_var"] - want["post_var"][0]) <= 2 * bar * want["second"][0]
    assert abs(got["post_sse"] - want["post_sse"][0]) <= bar * want["post_sse"][0]
    assert abs(got["ess"] - want["ess"][0]) <= B50 * K * want["ess"][0]


def test_a_subject_without_a_finite_term():
    z, a = np.array([-1.0, 0.0, 1.0]), np.zeros(3)
    x = np.stack([z, z, z], axis=1)
    sse = np.ones((3, 3))
    sse[:, 0] = [np.nan, np.inf, -np.inf]
    got = mr.marginal(z, a, x, sse, np.zeros(3), np.array([1.0, 0.0, 1.0]), 5, 0.4, 0.0, 1.0)
    assert list(got["n_bad"]) == [3, 3, 0]
    assert np.all(got["logml"][:2] == -np.inf) and np.isfinite(got["logml"][2])
    for k in ("post_mean", "post_var", "post_sse", "ess"):
        assert np.isnan(got[k][:2]).all() and np.isfinite(got[k][2])
    assert np.all(got["terms"][:, :2] == -np.inf)


@pytest.mark.parametrize("Q", list(range(1, 34)))
def test_gauss_hermite_rule_integrates_the_standard_normal(Q):
    from cude import api
    z, a = api.gauss_hermite_rule(Q)
    assert z.shape == a.shape == (Q,) and np.all(np.diff(z) > 0) and np.all(np.isfinite(a))
    w = np.exp(a - 0.5 * z * z) / math.sqrt(2.0 * math.pi)
    assert abs(math.fsum(w) - 1.0) <= 1e-13
    second = math.fsum(w * z * z)
    assert abs(second - (1.0 if Q > 1 else 0.0)) <= 1e-13
    if Q == 1:                                   # the Laplace value f(m) s sqrt(2 pi)
        assert z[0] == 0.0 and abs(a[0] - 0.5 * math.log(2.0 * math.pi)) <= 1e-15


def test_grid_rule_is_the_trapezoid_rule():
    from cude import api
    trapezoid = getattr(np, "trapezoid", None) or np.trapz
    f = lambda x: np.exp(-0.5 * (x - 0.3) ** 2) * (1.0 + 0.2 * np.sin(3.0 * x))
    for lo, hi, n in ((-7.4, 5.4, 4001), (-1.0, 2.0, 2), (0.0, 1.0, 17)):
        x, a = api.grid_rule(lo, hi, n)
        assert x.shape == a.shape == (n,) and x[0] == lo and x[-1] == hi
        want = trapezoid(f(x), x)
        assert abs(math.fsum(np.exp(a) * f(x)) - want) <= 1e-13 * abs(want)
    for bad in ((0.0, 1.0, 1), (1.0, 1.0, 5), (2.0, 1.0, 5)):
        with pytest.raises(ValueError):
            api.grid_rule(*bad)


def test_information_criteria_and_em_updates_on_hand_made_numbers():
    from cude import api
    ic = api.information_criteria(-120.5, 38, 35, 6)
    assert ic["aic"] == 241.0 + 76.0
    assert abs(ic["bic"] - (241.0 + 38 * math.log(210))) <= 1e-12
    assert abs(ic["bic_subjects"] - (241.0 + 38 * math.log(35))) <= 1e-12
    s2, mu, om2 = api.em_updates([1.0, 2.0, 3.0], [0.5, 0.25, 0.75], [2.0, 4.0, 6.0], 4)
    assert s2 == 1.0 and mu == 2.0
    assert abs(om2 - (0.5 + 2.0 / 3.0)) <= 1e-15            # mean variance 1/2 + spread of the means 2/3


def test_oracle_rules_differ_as_the_end_to_end_test_assumes():
    """The case of tests/test_gpu_marginal.py::test_end_to_end on the numpy oracle alone: the 33-node Gauss-Hermite rule
    at the MAP against the 4 001-point trapezoid over mu -/+ 8 Omega.  Measured: gaps 1.8e-15, 5.6e-2, 3.9e-14, 9.0e-9,
    1.2e-9, 1.4e-14 -- subject 1 has a second hump the rule does not see (posterior sd 0.30 on the grid, 0.073 by the
    rule) and is the one subject left out; at most one may be."""
    r = mr.end_to_end_oracle()
    gap = np.abs(r["q33"] - r["grid"])
    print("oracle gaps Q = 33:", gap, " Q = 1:", np.abs(r["q1"] - r["grid"]))
    assert np.sum(gap > 1e-6) <= 1 and np.sum(r["keep"]) >= 5
    assert np.max(gap[r["keep"]]) <= 1e-6
    assert np.all(np.abs(r["q1"] - r["grid"])[r["keep"]] > gap[r["keep"]])
