"""tests/vpc_ref.py -- the numpy restatement tests/test_gpu_vpc.py holds cude_vpc to -- against numpy's own quantile, and the
statistics of the check itself on the CPU oracle: a well-specified case stays inside its bands, a misspecified one does not.

The calibration's data seed is chosen here, on the CPU, so that the restatement alone meets the cap of 2 `outside` cells of
the R * 3; the shifted case (the random effects behind the data drawn 3 prior_sd off the fitted prior) must then show its
median outside in every row."""
import numpy as np
import pytest

import vpc_ref as vr

LEVELS9 = (0.0, 0.025, 0.05, 0.25, 0.5, 0.75, 0.95, 0.975, 1.0)
SIZES = list(range(1, 71)) + [117, 4096, 4097, 5000]
DATA_SEED = vr.CAL_DATA_SEED


def test_rule_3_is_numpy_quantile_to_the_bit():
    rng = np.random.default_rng(20251021)
    total = equal = 0
    for n in SIZES:
        base = rng.standard_normal(n)
        columns = [base * 1e-3, base, base * 1e3, np.round(base * 4.0) / 4.0, np.round(rng.standard_normal(n) * 1e3 + 50.0)]
        for x in columns:
            want = np.quantile(x, LEVELS9)
            got = np.array([vr.quantile(x, q) for q in LEVELS9])
            total += len(LEVELS9)
            equal += int(np.count_nonzero(got == want))
    print(f"rule 3 against numpy.quantile {np.__version__}: {equal} of {total} values equal")
    assert equal == total


def test_rule_3_is_api_quantile_lerp():
    from cude import api
    rng = np.random.default_rng(5)
    for n in (1, 2, 7, 64, 4097):
        x = np.sort(rng.standard_normal(n))
        ranks, lo, hi, g = api.quantile_ranks(LEVELS9, n)
        want = api.quantile_lerp(x[ranks[lo]], x[ranks[hi]], g)
        assert np.array_equal(want, [vr.quantile(x, q) for q in LEVELS9])


def test_membership_statuses_and_empty_groups():
    rng = np.random.default_rng(1)
    K, R, N = 5, 3, 12
    y, y_obs = rng.standard_normal((K, R, N)), rng.standard_normal((R, N))
    sigma = np.full(N, 0.1)
    groups = np.array([0, 0, 0, 0, 2, 2, 2, 2, 2, -1, 0, 2])
    y_obs[1, 10] = np.nan                       # BAD_OBS in group 0
    sigma[11] = np.inf                          # BAD_OBS in group 2
    y[3, 2, 5] = np.inf                         # simulation 3 fails for group 2
    r = vr.vpc(y, y_obs, sigma, groups, 3, (0.1, 0.5), (0.0, 1.0))
    assert list(r["n_members"]) == [4, 0, 5] and list(r["n_sims_used"]) == [K, K, K - 1]
    want = np.zeros(N, dtype=np.int32)
    want[9], want[10], want[11], want[5] = vr.NO_GROUP, vr.BAD_OBS, vr.BAD_OBS, vr.FAILED_SIMS
    assert np.array_equal(r["status"], want)
    assert np.all(np.isnan(r["observed"][1])) and np.all(np.isnan(r["simulated_ci"][1])) and np.all(np.isnan(r["simulated_q"][:, 1]))
    assert np.all(np.isnan(r["simulated_q"][3, 2])) and np.all(np.isfinite(r["simulated_q"][[0, 1, 2, 4], 2]))
    assert np.array_equal(r["observed"][0, :, 1], np.quantile(y_obs[:, :4], 0.5, axis=1))
    # ci levels 0 and 1 over the used simulations: the envelope of the simulated quantiles
    used = r["simulated_q"][[0, 1, 2, 4], 2]
    assert np.array_equal(r["simulated_ci"][2, :, :, 0], used.min(axis=0)) and np.array_equal(r["simulated_ci"][2, :, :, 1], used.max(axis=0))
    assert not r["outside"][1].any()


def test_group_labels_map_in_order_of_first_appearance():
    from cude import api
    ids, G, labels = api._vpc_groups(["T2DM", "NGT", "T2DM", "IGT", "NGT"], 5)
    assert list(ids) == [0, 1, 0, 2, 1] and G == 3 and labels == ["T2DM", "NGT", "IGT"]
    ids, G, labels = api._vpc_groups(np.array([2, -1, 0, 2]), 4)
    assert list(ids) == [2, -1, 0, 2] and G == 3 and labels is None and ids.dtype == np.int32
    assert api._vpc_groups(None, 4) == (None, 1, None)
    with pytest.raises(ValueError):
        api._vpc_groups([0, 1], 3)


def test_calibration_a_well_specified_case_stays_inside_and_a_shifted_one_does_not():
    cs, _, _, y, r = vr.calibration(DATA_SEED)
    R = cs["R"]
    assert y.shape == (vr.K_CAL, R, vr.N_CAL) and r["n_members"][0] == vr.N_CAL and r["n_sims_used"][0] == vr.K_CAL
    n_out = int(np.count_nonzero(r["outside"]))
    print(f"well specified (data seed {DATA_SEED}): {n_out} of {R * 3} cells outside")
    assert r["outside"].shape == (1, R, 3) and n_out <= 2
    # the bands bracket their own medians and are ordered
    ci = r["simulated_ci"]
    assert np.all(ci[..., 0] <= ci[..., 1]) and np.all(ci[..., 1] <= ci[..., 2])
    assert np.all(ci[:, :, 0, 1] < ci[:, :, 1, 1]) and np.all(ci[:, :, 1, 1] < ci[:, :, 2, 1])
    _, _, _, _, s = vr.calibration(DATA_SEED, obs_shift=3.0)
    print(f"shifted by 3 prior_sd: {int(np.count_nonzero(s['outside']))} of {R * 3} cells outside; median rows {s['outside'][0, :, 1]}")
    assert np.all(s["outside"][0, :, 1])
