"""The rule of cude_profile_intervals (include/cude.h), restated in tests/profile_ref.py, on the C oracle's profiles -- no GPU.

  * n_rounds = 0 is the reference's find_confidence_intervals (cude/api.py's mirror of src/likelihood-profiles.jl:34-59) row
    by row, for all three targets, -/+Inf ends and the empty case included;
  * after r rounds every closed end brackets the crossing: F(in) <= thr < F(out), |in - out| = grid spacing / (m + 1)^r;
  * the chunked reduction is the unchunked one, exactly;
  * every status flag occurs in the case list (which case produced which is printed, and recorded below).

Recorded (seeds of conftest): DISCONNECTED comes from "cpep-beta" (centre = the case's beta, sigma 0.3: profiles with a second
basin inside the threshold) and from "supp-theta"; BELOW_CENTER from the same two (their centres are no minimisers);
LOWER/UPPER_OPEN from "cpep-narrow"; EMPTY from "cpep-tiny" (centre = the refined minimiser between two grid points,
sigma 1e-4); CENTER_FAILED from "cpep-nan" (subject 3's centre is NaN)."""
import os
import re

import numpy as np
import pytest

from conftest import make_cpep_case, make_supp_case
import profile_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGETS = ("cantelli95", "cantelli90", "raue95")

# name -> (model, n_points, range, centre, sigma, (pw, pc))
CASES = {
    "cpep-argmin": ("cpep", 41, (-4.0, 3.0), "argmin", 0.05, (0.0, 0.0)),
    "cpep-beta": ("cpep", 41, (-4.0, 3.0), "given", 0.3, (0.0, 0.0)),
    "cpep-penalised": ("cpep", 37, (-4.0, 3.0), "argmin", 0.1, (0.35, -0.6)),
    "cpep-narrow": ("cpep", 11, (-1.0, -0.9), "given", 1.0, (0.0, 0.0)),
    "cpep-tiny": ("cpep", 41, (-4.0, 3.0), "refined", 1e-4, (0.0, 0.0)),
    "cpep-nan": ("cpep", 41, (-4.0, 3.0), "nan3", 0.05, (0.0, 0.0)),
    "supp-theta": ("supp", 41, (-6.0, 4.0), "given", 0.3, (0.0, 0.0)),
    "supp-argmin": ("supp", 37, (-6.0, 4.0), "argmin", 1.0, (0.35, -0.6)),
}


@pytest.fixture(scope="module")
def oracle():
    """model -> (evaluator, the case's own conditional parameters); profiles are cached per (model, grid)."""
    c, s = make_cpep_case(24, (2, 4, 2)), make_supp_case(16)
    evs = {"cpep": (pr.cpep_evaluator(c), c["beta"]), "supp": (pr.supp_evaluator(s), s["theta"])}
    cache = {}

    def get(name):
        model, K, box, kind, sigma, (pw, pc) = CASES[name]
        ev, given = evs[model]
        N = given.size
        values = np.linspace(box[0], box[1], K)
        key = (model, K, box)
        if key not in cache:
            cache[key] = np.stack([ev(np.full(N, v)) for v in values])
        prof = cache[key]
        k = np.argmin(pr.objective(prof, values[:, None], pw, pc), axis=0)
        if kind == "given":
            center = given.copy()
        elif kind == "argmin":
            center = values[k]
        elif kind == "nan3":
            center = values[k].copy()
            center[3] = np.nan
        else:                                   # golden section inside the bracket around the grid's argmin
            k = np.clip(k, 1, K - 2)
            lo, hi, gr = values[k - 1], values[k + 1], (np.sqrt(5.0) - 1.0) / 2.0
            for _ in range(40):
                a, b = hi - gr * (hi - lo), lo + gr * (hi - lo)
                left = ev(a) < ev(b)
                lo, hi = np.where(left, lo, a), np.where(left, b, hi)
            center = 0.5 * (lo + hi)
        return ev, values, prof, center, sigma, pw, pc
    return get


def _delta(sigma, target):
    from cude import api
    return 2.0 * sigma ** 2 * api._CI_THRESHOLDS[target]


@pytest.mark.parametrize("name", list(CASES))
def test_grid_stage_is_find_confidence_intervals(oracle, name):
    from cude import api
    ev, values, prof, center, sigma, pw, pc = oracle(name)
    N = center.size
    with np.errstate(all="ignore"):
        sse_c = ev(center)
    F = pr.objective(prof, values[:, None], pw, pc)
    Fc = pr.objective(sse_c, center, pw, pc)
    for target in TARGETS:
        r = pr.intervals(ev, values, center, _delta(sigma, target), pw, pc, profile=prof, sse_center=sse_c)
        for i in range(N):
            nll_min = Fc[i] / (2 * sigma ** 2) if np.isfinite(Fc[i]) else np.nan
            try:
                lo, hi = api.find_confidence_intervals(F[:, i] / (2 * sigma ** 2), nll_min, values, target=target)
            except ValueError:
                assert r["status"][i] & (pr.EMPTY | pr.CENTER_FAILED) and np.isnan(r["lower"][i]) and np.isnan(r["upper"][i])
                assert r["n_inside"][i] == 0
                continue
            assert (r["lower"][i], r["upper"][i]) == (lo, hi), (name, target, i)
            assert bool(r["status"][i] & pr.LOWER_OPEN) == (lo == -np.inf)
            assert bool(r["status"][i] & pr.UPPER_OPEN) == (hi == np.inf)
            assert r["n_inside"][i] == np.count_nonzero(F[:, i] <= Fc[i] + _delta(sigma, target))
        assert np.array_equal(r["argmin"], values[np.argmin(F, axis=0)]) and np.array_equal(r["min"], F.min(axis=0))
    # an unknown target is raue95, as in the reference
    assert api._CI_THRESHOLDS.get("no-such-target", api._CI_THRESHOLDS["raue95"]) == api._CI_THRESHOLDS["raue95"]


@pytest.mark.parametrize("m,rounds", [(1, 6), (3, 4), (16, 2)])
@pytest.mark.parametrize("name", ["cpep-argmin", "cpep-beta", "supp-theta", "supp-argmin"])
def test_rounds_bracket_the_crossing(oracle, name, m, rounds):
    ev, values, prof, center, sigma, pw, pc = oracle(name)
    r = pr.intervals(ev, values, center, _delta(sigma, "cantelli95"), pw, pc, rounds=rounds, sections=m, profile=prof)
    g = pr.intervals(ev, values, center, _delta(sigma, "cantelli95"), pw, pc, profile=prof)
    lo_out, lo_in, hi_in, hi_out = r["brackets"]
    width = (values[1] - values[0]) / (m + 1) ** rounds
    # every round forms a point by one subtraction, product, quotient and sum of numbers no larger than max |values|
    tol = 8 * rounds * np.finfo(float).eps * np.max(np.abs(values))
    closed = 0
    for out, inn, grid_in in ((lo_out, lo_in, g["lower"]), (hi_out, hi_in, g["upper"])):
        act = ~np.isnan(out)
        assert np.array_equal(act, np.isfinite(grid_in))
        assert np.array_equal(inn[~act], grid_in[~act], equal_nan=True)         # open / empty ends are not written
        if not act.any():
            continue
        x_in, x_out = np.where(act, inn, center), np.where(act, out, center)
        F_in, F_out = pr.objective(ev(x_in), x_in, pw, pc), pr.objective(ev(x_out), x_out, pw, pc)
        assert np.all(F_in[act] <= r["thr"][act]) and np.all(F_out[act] > r["thr"][act])
        assert np.all(np.abs(np.abs(inn - out)[act] - width) <= tol)
        # the refined end lies inside the grid's bracket, on the inner side of the outer grid point
        assert np.all(np.abs(inn[act] - grid_in[act]) < values[1] - values[0])
        closed += int(act.sum())
    print(f"{name} m={m} rounds={rounds}: {closed} closed ends, final width {width:.3e}")
    assert closed > 0
    assert np.array_equal(r["status"], g["status"]) and np.array_equal(r["n_inside"], g["n_inside"])


@pytest.mark.parametrize("name", list(CASES))
def test_chunked_reduction_is_the_unchunked_one(oracle, name):
    ev, values, prof, center, sigma, pw, pc = oracle(name)
    with np.errstate(all="ignore"):
        sse_c = ev(center)
    want = pr.intervals(ev, values, center, _delta(sigma, "cantelli90"), pw, pc, profile=prof, sse_center=sse_c)
    for chunk in (1, 5, 8, len(values) - 1):
        got = pr.intervals(ev, values, center, _delta(sigma, "cantelli90"), pw, pc, profile=prof, sse_center=sse_c, chunk=chunk)
        for k in ("lower", "upper", "argmin", "min", "center_objective", "n_inside", "status"):
            assert np.array_equal(got[k], want[k], equal_nan=True), (name, chunk, k)
    a = pr.intervals(ev, values, None, 0.0, pw, pc, profile=prof, argmin_only=True, chunk=8)
    assert np.array_equal(a["argmin"], want["argmin"]) and np.array_equal(a["min"], want["min"])


def test_every_status_flag_occurs(oracle):
    seen = {}
    for name in CASES:
        ev, values, prof, center, sigma, pw, pc = oracle(name)
        r = pr.intervals(ev, values, center, _delta(sigma, "cantelli95"), pw, pc, profile=prof)
        for flag in (pr.LOWER_OPEN, pr.UPPER_OPEN, pr.DISCONNECTED, pr.EMPTY, pr.CENTER_FAILED, pr.BELOW_CENTER):
            if np.any(r["status"] & flag):
                seen.setdefault(flag, []).append(name)
        print(name, {int(s): int(np.count_nonzero(r["status"] == s)) for s in np.unique(r["status"])})
    print("flag -> cases:", seen)
    assert sorted(seen) == [1, 2, 4, 8, 16, 32]
    assert "cpep-beta" in seen[pr.DISCONNECTED] and "supp-theta" in seen[pr.DISCONNECTED]
    assert "cpep-narrow" in seen[pr.LOWER_OPEN] and "cpep-narrow" in seen[pr.UPPER_OPEN]
    assert seen[pr.EMPTY] == ["cpep-tiny"] and seen[pr.CENTER_FAILED] == ["cpep-nan"]
    assert "cpep-beta" in seen[pr.BELOW_CENTER]


def test_all_values_non_finite_give_index_zero():
    values = np.linspace(0.0, 1.0, 5)
    prof = np.full((5, 2), np.nan)
    prof[:, 1] = [3.0, 1.0, 1.0, 2.0, np.inf]
    r = pr.intervals(None, values, np.array([0.5, 0.5]), 0.5, profile=prof, sse_center=np.array([1.0, 1.0]))
    assert r["argmin"][0] == values[0] and r["min"][0] == np.inf and r["status"][0] == pr.EMPTY
    assert r["argmin"][1] == values[1] and (r["lower"][1], r["upper"][1]) == (values[1], values[2]) and r["n_inside"][1] == 2


def test_constants_and_defaults_agree_across_the_layers():
    import inspect
    from cude import api, engine, _lib
    hdr = open(os.path.join(ROOT, "include", "cude.h")).read()
    bits = {k: int(v) for k, v in re.findall(r"#define CUDE_CI_(\w+)\s+(\d+)", hdr)}
    assert bits == dict(LOWER_OPEN=1, UPPER_OPEN=2, DISCONNECTED=4, EMPTY=8, CENTER_FAILED=16, BELOW_CENTER=32)
    for k, v in bits.items():
        assert getattr(engine, "CI_" + k) == v and getattr(pr, k) == v
    assert "cude_profile_intervals" in _lib.exported_symbols()
    eng = inspect.signature(engine.Engine.profile_intervals).parameters
    for fn in (api.profile_confidence_intervals, api.suppression_profile_intervals):
        p = inspect.signature(fn).parameters
        assert (p["steps"].default, p["target"].default, p["rounds"].default, p["n_steps"].default) == (1000, "cantelli95", 0, None)
        assert p["sections"].default == eng["sections"].default == inspect.signature(pr.intervals).parameters["sections"].default
    jl = open(os.path.join(ROOT, "conditional-ude_amd", "julia", "CUDEHip.jl")).read()
    assert re.search(r"function profile_confidence_intervals\([^)]*;\s*steps = 1000, target = \"cantelli95\", rounds = 0,\s*"
                     r"sections = %d" % p["sections"].default, jl)
    for needle in ("\"profile_chunk\"", "CUDE_PROFILE_CHUNK"):
        assert needle in hdr and needle in open(os.path.join(ROOT, "conditional-ude_amd", "csrc", "cude_ctx.h")).read()
