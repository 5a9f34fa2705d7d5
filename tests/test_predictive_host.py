"""Host side of the posterior-predictive bands: the declarations of the two entry points in every binding, the quantile
rule of the mirrors against numpy.quantile, and the numpy restatement (tests/predictive_ref.py) the GPU tests compare the
device with -- its mean, its NaN rule and its best-of-sets reduction on the C oracle's SSEs."""
import math
import os
import re

import numpy as np
import pytest

from conftest import make_cpep_case
import predictive_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cude_predictive_bands", "cude_evaluate_conditional_sets")


def test_every_binding_declares_the_entry_points():
    header = open(os.path.join(ROOT, "include", "cude.h")).read()
    julia = open(os.path.join(ROOT, "conditional-ude_amd", "julia", "CUDEHip.jl")).read()
    from cude import _lib
    for name in NEW:
        assert re.search(r"int32_t\s+%s\s*\(" % name, header), name
        assert name in _lib.exported_symbols(), name
        assert (":%s," % name) in julia, name
    for needle in ('"predictive_subjects"', '"predictive_times"', "CUDE_PREDICTIVE_SUBJECTS", "CUDE_PREDICTIVE_TIMES"):
        assert needle in header, needle
    from cude.engine import Engine
    assert hasattr(Engine, "predictive_bands") and hasattr(Engine, "evaluate_conditional_sets")


@pytest.mark.parametrize("K", [1, 2, 37, 200])
def test_quantile_ranks_and_lerp_match_numpy(K):
    """x_lo + g (x_hi - x_lo) (api.quantile_lerp) on the order statistics quantile_ranks asks for against numpy.quantile's default (type 7).
    rtol 1e-14: either side makes at most three roundings of numbers no larger than the two neighbours, all positive."""
    from cude import api
    rng = np.random.default_rng(100 + K)
    levels = [0.0, 0.025, 0.5, 0.5, 0.3, 0.975, 1.0, 1.0 / 3.0]
    ranks, lo, hi, g = api.quantile_ranks(levels, K)
    assert ranks.dtype == np.int32 and np.all(np.diff(ranks) > 0) and ranks[0] >= 0 and ranks[-1] <= K - 1
    assert np.all((g >= 0) & (g < 1)) and len(lo) == len(hi) == len(g) == len(levels)
    h = (K - 1) * np.asarray(levels)
    assert np.array_equal(ranks[lo], np.floor(h).astype(int)) and np.array_equal(ranks[hi], np.minimum(ranks[lo] + 1, K - 1))
    v = rng.lognormal(size=(K, 50))
    srt = np.sort(v, axis=0)[ranks]                          # what the device returns
    got = api.quantile_lerp(srt[lo], srt[hi], g[:, None])
    plain = srt[lo] + g[:, None] * (srt[hi] - srt[lo])           # the rule as written: the same number to rounding
    assert np.max(np.abs(got - plain) / srt[hi]) <= 4 * 2.0 ** -53
    np.testing.assert_allclose(got, np.quantile(v, levels, axis=0), rtol=1e-14, atol=0)


def test_quantile_ranks_rejects_levels_outside_the_unit_interval():
    from cude import api
    for bad in ([-0.1], [1.5], [float("nan")]):
        with pytest.raises(ValueError):
            api.quantile_ranks(bad, 10)


@pytest.mark.parametrize("K", [1, 2, 37, 200])
def test_sequential_mean_against_fsum(K):
    """K - 1 adds of positive numbers: each rounds a partial sum no larger than the total, so the error is below
    K 2^-53 relative."""
    v = np.random.default_rng(K).lognormal(size=(K, 3, 40))
    got = pr.sequential_mean(v)
    for j in range(3):
        for i in range(40):
            want = math.fsum(v[:, j, i]) / K
            assert abs(got[j, i] - want) <= K * 2.0 ** -53 * want


def test_bands_nan_rule_and_selection():
    rng = np.random.default_rng(5)
    K, T, N = 37, 4, 6
    v = rng.lognormal(size=(K, T, N))
    ranks = [0, 1, K // 2, K - 2, K - 1]
    clean = pr.bands(v, ranks)
    assert np.array_equal(clean["order"], np.sort(v, axis=0)[ranks].transpose(2, 1, 0))
    assert np.isin(clean["order"], v).all()                              # a selection: the inputs' own bits
    assert np.array_equal(clean["order"][:, :, 0], v.min(axis=0).T) and np.array_equal(clean["order"][:, :, -1], v.max(axis=0).T)
    assert not clean["bad_sets"].any()
    w = v.copy()
    w[3, 1:, 2] = np.nan                                                # set 3 of subject 2: NaN from time 1 on
    w[5, 2, 2] = np.inf                                                 # set 5: one infinite value
    w[7, 0, 4] = -np.inf
    got = pr.bands(w, ranks)
    assert np.isnan(got["order"][2, 1:]).all() and np.isnan(got["mean"][2, 1:]).all()
    assert np.array_equal(got["order"][2, 0], clean["order"][2, 0]) and got["mean"][2, 0] == clean["mean"][2, 0]
    assert np.isnan(got["order"][4, 0]).all() and np.array_equal(got["order"][4, 1:], clean["order"][4, 1:])
    assert list(got["bad_sets"]) == [0, 0, 2, 0, 1, 0]
    others = [0, 1, 3, 5]
    assert np.array_equal(got["order"][others], clean["order"][others]) and np.array_equal(got["mean"][others], clean["mean"][others])
    # what numpy.quantile says of such a column
    assert np.isnan(np.quantile(w[:, 1, 2], 0.5))
    only_mean = pr.bands(v, [])
    assert only_mean["order"].shape == (N, T, 0) and np.array_equal(only_mean["mean"], clean["mean"])


def test_best_of_sets_on_the_oracle_sses():
    import c_oracle as co
    arch = (2, 4, 2)
    c = make_cpep_case(24, arch)
    N, K = 24, 9
    x = c["beta"][None, :] + 0.4 * np.random.default_rng(11).standard_normal((K, N))
    x[4] = x[1]                                  # a duplicated set: the tie goes to the first
    x[6] = np.nan                                # a set of NaN
    sse = np.stack([co.cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"], arch, c["nn"], np.nan_to_num(xk), 30, 2,
                            want_grad=False)["sse"] for xk in x])
    sse[6] = np.nan
    sse[:, 5] = np.inf                           # a subject with no finite value
    assert np.array_equal(sse[4], sse[1])
    for pw, pc in ((0.0, 0.0), (0.35, -0.6)):
        idx, best = pr.best_of_sets(sse, x, pw, pc)
        f = sse + pw * (x - pc) ** 2
        f[~np.isfinite(f)] = np.inf
        assert idx.dtype == np.int32
        assert idx[5] == 0 and best[5] == np.inf
        ok = np.arange(N) != 5
        assert np.array_equal(best[ok], f.min(axis=0)[ok]) and np.array_equal(idx[ok], f.argmin(axis=0)[ok])
        assert not np.any(idx == 4) and not np.any(idx == 6)
        assert np.any(idx == 1)                  # the duplicated set does win somewhere -- as set 1
