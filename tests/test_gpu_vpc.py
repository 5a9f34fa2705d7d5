"""cude_vpc on the device (csrc/cude_vpc.hip): the visual predictive check by subject group, against

  * the rules restated in numpy (tests/vpc_ref.py, which tests/test_vpc_host.py holds to numpy.quantile), fed the simulated
    observations cude_npde returns from the same seed, first_rep, sets and noise (rule 1: the same bits);
  * itself: the sorting tile against the radix select (option "vpc_select"), every split over simulations ("vpc_sims"),
    a clean run against one with failed simulations or a bad observation;
  * the calibration study of tests/test_vpc_host.py through the api mirror.

Every comparison of doubles is numpy.array_equal on values with NaNs matched by position (vpc_ref.same): the quantiles are
selected order statistics and five operations rounded one by one, so nothing is left to a tolerance.

Shapes: N = 67 (two solve workgroups), T = 6 (R = 5) or T = 3, K = 3 ... 257; one population of 5100 subjects for the column
lengths around the tile's limit of 4096.

Not reachable from outside: CUDE_ERR_STATE under stream capture (the library captures inside cude_adam_run only)."""
import numpy as np
import pytest
import torch  # noqa: F401

import vpc_ref as vr

pytestmark = pytest.mark.gpu

LEVELS, CI = (0.05, 0.5, 0.95), (0.025, 0.5, 0.975)
DOUBLES = ("observed", "simulated_q", "simulated_ci")


def _groups67():
    """Groups of sizes 1, 2 and the rest of 67 subjects, three subjects left out."""
    g = np.full(67, 2, dtype=np.int32)
    g[5] = 0
    g[[9, 40]] = 1
    g[[0, 33, 66]] = -1
    return g


def _check(label, got, sims, y_obs, sigma, groups, G, levels=LEVELS, ci=CI):
    """The device's outputs against the restatement on `sims`; rule 6 on the device's own simulated quantiles."""
    ref = vr.vpc(sims, y_obs, sigma, groups, G, levels, ci, sim_q=got["simulated_q"])
    for k in ("simulated_q", "observed", "simulated_ci", "n_members", "n_sims_used", "status"):
        assert vr.same(got[k], ref[k]), (label, k)
    return ref


def _all_same(a, b, label=""):
    for k in a:
        assert vr.same(a[k], b[k]), (label, k)


# ----------------------------------------------------------------------------- 1. simulated quantiles to the bit
@pytest.mark.parametrize("name", ["cpep-2441", "supp-4355"])
def test_quantiles_are_the_restatement_on_npdes_sims(name):
    cs = vr.case(name, 67)
    K, groups = 7, _groups67()
    eng = vr.make_engine(cs)
    eng.set_rng(0xC0FFEE)
    kw = dict(prior_mean=cs["prior_mean"], prior_sd=cs["prior_sd"], first_rep=11, state=cs["state"])
    sims = eng.npde(cs["sigma"], K, want_sims=True, want_decorrelated=False, **kw)["sims"]
    got = eng.vpc(cs["sigma"], K, groups=groups, n_groups=3, levels=LEVELS, ci_levels=CI, **kw)
    assert eng.n_failed() == 0
    # host draws as well
    cond, noise = vr.draws(cs, K)
    sims_h = eng.npde(cs["sigma"], K, cond, noise=noise, state=cs["state"], want_sims=True, want_decorrelated=False)["sims"]
    got_h = eng.vpc(cs["sigma"], K, cond, noise=noise, state=cs["state"], groups=groups, n_groups=3)
    eng.close()
    assert np.all(np.isfinite(sims)) and not np.array_equal(sims, sims_h)
    ref = _check(name, got, sims, cs["y_obs"], cs["sigma"], groups, 3)
    _check(name + " host draws", got_h, sims_h, cs["y_obs"], cs["sigma"], groups, 3)
    assert list(got["n_members"]) == [1, 2, 61] and list(got["n_sims_used"]) == [K] * 3
    assert np.array_equal(got["status"], np.where(groups < 0, vr.NO_GROUP, 0))
    assert got["observed"].shape == (3, 5, 3) and got["simulated_ci"].shape == (3, 5, 3, 3) and got["simulated_q"].shape == (K, 3, 5, 3)
    # a group of one: every quantile is that subject's value
    assert np.array_equal(got["observed"][0], np.repeat(cs["y_obs"][:, 5, None], 3, axis=1))
    assert np.array_equal(ref["simulated_q"][:, 0, :, 1], sims[:, :, 5])


# ----------------------------------------------------------------------------- 2. every column length that changes the path
N_BIG = 5100


@pytest.fixture(scope="module")
def big():
    cs = vr.case("cpep-2441", N_BIG, 3)
    K = 3
    cond, noise = vr.draws(cs, K)
    eng = vr.make_engine(cs)
    sims = eng.npde(cs["sigma"], K, cond, noise=noise, want_sims=True, want_decorrelated=False)["sims"]
    yield cs, eng, cond, noise, sims
    eng.close()


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 129, 4096, 4097, 5000])
def test_every_column_length(big, n):
    """n members scattered over 5100 subjects: tile columns of 1 ... 4096 values (padded lengths 1 ... 4096, 64 ... 2 columns per
    tile), the select kernel from 4097 on -- and for every n the tile allows, the select kernel as well."""
    cs, eng, cond, noise, sims = big
    K = 3
    rng = np.random.default_rng(n)
    groups = np.full(N_BIG, -1, dtype=np.int32)
    groups[rng.choice(N_BIG, size=n, replace=False)] = 0
    levels = (0.0, 0.05, 0.31, 0.5, 0.77, 0.95, 1.0)
    kw = dict(noise=noise, groups=groups, n_groups=1, levels=levels, ci_levels=CI)
    got = eng.vpc(cs["sigma"], K, cond, **kw)
    _check(f"n={n}", got, sims, cs["y_obs"], cs["sigma"], groups, 1, levels=levels)
    assert got["n_members"][0] == n and np.all(np.isfinite(got["simulated_q"]))
    if n <= 4096:
        eng.set_option("vpc_select", 1)
        try:
            sel = eng.vpc(cs["sigma"], K, cond, **kw)
        finally:
            eng.set_option("vpc_select", 0)
        _all_same(got, sel, f"n={n} select")


# ----------------------------------------------------------------------------- 3. negative values and ties
@pytest.mark.parametrize("select", [0, 1])
def test_negative_values_and_ties(select):
    """sigma = 4 around c-peptide values of order 1: the key's negative branch.  Subjects 7 and 8 share every input and have
    sigma = 0: their simulated observations are equal, and in a group of three the median's rank 1 is one of the pair; in
    the group of all the others the pair is two equal values somewhere in a column of 64."""
    cs = dict(vr.case("cpep-2441", 67))
    for key in ("G", "obs", "age", "t2dm"):
        cs[key] = cs[key].copy()
        cs[key][8] = cs[key][7]
    y_obs = cs["obs"][:, 1:].T.copy()
    K = 9
    cond, noise = vr.draws(cs, K)
    cond[:, 8] = cond[:, 7]
    sigma = np.full(67, 4.0)
    sigma[[7, 8]] = 0.0
    trio = np.full(67, -1, dtype=np.int32)
    trio[[7, 8, 20]] = 0
    rest = np.zeros(67, dtype=np.int32)
    rest[[1, 2, 3]] = 1
    eng = vr.make_engine(cs, options=(("vpc_select", select),))
    sims = eng.npde(sigma, K, cond, noise=noise, want_sims=True, want_decorrelated=False)["sims"]
    assert np.count_nonzero(sims < 0) >= sims.size / 4
    assert np.array_equal(sims[:, :, 7], sims[:, :, 8])
    levels = (0.0, 0.25, 0.5, 0.75, 1.0)
    for label, groups, G in (("trio", trio, 1), ("rest", rest, 2)):
        got = eng.vpc(sigma, K, cond, noise=noise, groups=groups, n_groups=G, levels=levels, ci_levels=CI)
        _check(label, got, sims, y_obs, sigma, groups, G, levels=levels)
        if label == "trio":
            # the median of (a, a, b) is a
            assert np.array_equal(got["simulated_q"][:, 0, :, 2], sims[:, :, 7])
            assert np.any(got["simulated_q"] < 0)
    eng.close()


# ----------------------------------------------------------------------------- 4. chunk independence
@pytest.mark.parametrize("name", ["cpep-2441", "supp-4355"])
def test_every_split_over_simulations_gives_the_same_bits(name):
    cs = vr.case(name, 67)
    K, groups = 7, _groups67()
    cond, noise = vr.draws(cs, K)
    eng = vr.make_engine(cs)
    eng.set_rng(99)
    dev = dict(prior_mean=cs["prior_mean"], prior_sd=cs["prior_sd"], first_rep=5, state=cs["state"], groups=groups, n_groups=3)
    host = dict(noise=noise, state=cs["state"], groups=groups, n_groups=3)
    whole_d, whole_h = eng.vpc(cs["sigma"], K, **dev), eng.vpc(cs["sigma"], K, cond, **host)
    for per_pass in (1, 2, 7):
        eng.set_option("vpc_sims", per_pass)
        _all_same(whole_d, eng.vpc(cs["sigma"], K, **dev), f"device draws, {per_pass} per pass")
        _all_same(whole_h, eng.vpc(cs["sigma"], K, cond, **host), f"host draws, {per_pass} per pass")
    eng.close()
    assert not vr.same(whole_d["simulated_q"], whole_h["simulated_q"])


# ----------------------------------------------------------------------------- 5. stage 2 geometry
@pytest.mark.parametrize("K", [2, 5, 64, 65, 257])
def test_every_count_of_simulations(K):
    """The interval's tile: padded lengths 2, 8, 64, 128, 512 (64 ... 16 columns per tile) over G R L = 45 columns."""
    cs = vr.case("cpep-2441", 67)
    groups = _groups67()
    cond, noise = vr.draws(cs, K)
    eng = vr.make_engine(cs)
    got = eng.vpc(cs["sigma"], K, cond, noise=noise, groups=groups, n_groups=3)
    env = eng.vpc(cs["sigma"], K, cond, noise=noise, groups=groups, n_groups=3, ci_levels=(0.0, 1.0))
    eng.close()
    ci = vr.intervals(got["simulated_q"], np.zeros((K, 3), dtype=bool), got["n_members"], CI)
    assert vr.same(got["simulated_ci"], ci)
    assert np.all(got["simulated_ci"][..., 0] <= got["simulated_ci"][..., 1]) and np.all(got["n_sims_used"] == K)
    # the levels 0 and 1: the envelope
    assert np.array_equal(env["simulated_ci"][..., 0], got["simulated_q"].min(axis=0))
    assert np.array_equal(env["simulated_ci"][..., 1], got["simulated_q"].max(axis=0))


# ----------------------------------------------------------------------------- 6. failed simulations
def test_a_failed_simulation_is_left_out_for_its_group_only():
    """Suppression solves carry a NaN conditional parameter to every output (tests/test_gpu_npde.py)."""
    cs = vr.case("supp-4355", 67)
    K, groups = 12, _groups67()
    cond, noise = vr.draws(cs, K)
    eng = vr.make_engine(cs)
    kw = dict(noise=noise, state=cs["state"], groups=groups, n_groups=3)
    clean = eng.vpc(cs["sigma"], K, cond, **kw)
    assert eng.n_failed() == 0
    bad = cond.copy()
    bad[4, 40] = np.nan                          # subject 40: group 1
    bad[6, 33] = np.nan                          # subject 33 is in no group: nobody notices
    for per_pass in (0, 5):
        eng.set_option("vpc_sims", per_pass)
        got = eng.vpc(cs["sigma"], K, bad, **kw)
        assert eng.n_failed() == 1
        assert list(got["n_sims_used"]) == [K, K - 1, K] and list(got["n_members"]) == [1, 2, 61]
        want = np.where(groups < 0, vr.NO_GROUP, 0)
        want[40] = vr.FAILED_SIMS
        assert np.array_equal(got["status"], want)
        assert np.all(np.isnan(got["simulated_q"][4, 1])) and np.all(np.isfinite(np.delete(got["simulated_q"], 4, axis=0)))
        for k in DOUBLES:
            a, b = np.moveaxis(got[k], 1 if k == "simulated_q" else 0, 0), np.moveaxis(clean[k], 1 if k == "simulated_q" else 0, 0)
            assert vr.same(a[[0, 2]], b[[0, 2]]), k
        # group 1: the other eleven simulations as in the clean run, the interval over those eleven
        assert np.array_equal(np.delete(got["simulated_q"][:, 1], 4, axis=0), np.delete(clean["simulated_q"][:, 1], 4, axis=0))
        sims = eng.npde(cs["sigma"], K, bad, noise=noise, state=cs["state"], want_sims=True, want_decorrelated=False)["sims"]
        _check("failed", got, sims, cs["y_obs"], cs["sigma"], groups, 3)
    eng.close()


# ----------------------------------------------------------------------------- 7. a bad observation, an empty group
def test_a_bad_observation_leaves_its_subject_out():
    cs = vr.case("cpep-2441", 67)
    K = 7
    cond, noise = vr.draws(cs, K)
    obs = cs["obs"].copy()
    obs[50, 2] = np.nan
    y_obs = obs[:, 1:].T.copy()
    groups = _groups67()
    groups[groups == 2] = 3                      # group 2 of 4 is empty
    eng = vr.make_engine(dict(cs, obs=obs))
    kw = dict(noise=noise, n_groups=4)
    got = eng.vpc(cs["sigma"], K, cond, groups=groups, **kw)
    assert eng.n_failed() == 1
    out = groups.copy()
    out[50] = -1
    ref = eng.vpc(cs["sigma"], K, cond, groups=out, **kw)
    assert eng.n_failed() == 0
    sims = eng.npde(cs["sigma"], K, cond, noise=noise, want_sims=True, want_decorrelated=False)["sims"]
    # a non-finite sigma counts alike
    sg = cs["sigma"].copy()
    sg[50] = np.inf
    eng2 = vr.make_engine(cs)
    inf = eng2.vpc(sg, K, cond, groups=groups, **kw)
    eng2.close()
    eng.close()
    want = np.where(groups < 0, vr.NO_GROUP, 0)
    want[50] = vr.BAD_OBS
    assert np.array_equal(got["status"], want) and np.array_equal(inf["status"], want)
    assert ref["status"][50] == vr.NO_GROUP
    for k in DOUBLES + ("n_members", "n_sims_used"):
        assert vr.same(got[k], ref[k]), k
    assert list(got["n_members"]) == [1, 2, 0, 60] and list(inf["n_members"]) == [1, 2, 0, 60]
    assert got["n_sims_used"][2] == K
    for k in DOUBLES:
        g_axis = 1 if k == "simulated_q" else 0
        assert np.all(np.isnan(np.take(got[k], 2, axis=g_axis))), k
        assert np.all(np.isfinite(np.delete(got[k], 2, axis=g_axis))), k
    _check("bad observation", got, sims, y_obs, cs["sigma"], groups, 4)


# ----------------------------------------------------------------------------- 8. adaptive mode
@pytest.mark.parametrize("name", ["cpep-2441", "supp-4355"])
def test_adaptive_mode(name):
    from cude._lib import CudeError
    cs = vr.case(name, 67)
    K, groups = 7, _groups67()
    cond, noise = vr.draws(cs, K)
    eng = vr.make_engine(cs, n_steps=0)
    sims = eng.npde(cs["sigma"], K, cond, noise=noise, state=cs["state"], want_sims=True, want_decorrelated=False)["sims"]
    eng.set_params(None, cond[0])
    eng.loss_grad()
    eng.adaptive_steps(0)
    got = eng.vpc(cs["sigma"], K, cond, noise=noise, state=cs["state"], groups=groups, n_groups=3)
    with pytest.raises(CudeError) as e:
        eng.adaptive_steps(0)
    assert e.value.status == -3
    eng.set_option("vpc_sims", 3)
    _all_same(got, eng.vpc(cs["sigma"], K, cond, noise=noise, state=cs["state"], groups=groups, n_groups=3), "split")
    eng.close()
    _check(name + " adaptive", got, sims, cs["y_obs"], cs["sigma"], groups, 3)


# ----------------------------------------------------------------------------- 9. errors and side effects
def test_errors_side_effects_and_outputs_that_can_be_omitted():
    from cude._lib import CudeError
    from cude.engine import Engine, _ptr
    cs = vr.case("cpep-2441", 67)
    N, R, K = cs["N"], cs["R"], 6
    cond, noise = vr.draws(cs, K)
    groups = _groups67()
    eng = vr.make_engine(cs)
    eng.set_rng(7)
    eng.set_params(None, cond[0])
    nn0, cond0 = eng.get_params()
    stream0 = eng.rng_draws(0, 2)
    chain0 = eng.mh_chain(None, None, 0.4, -0.6, 0.9, 0.3, n_mc=2)[1]
    eng.set_rng(7)
    eng.set_params(None, cond[0])
    full = eng.vpc(cs["sigma"], K, cond, noise=noise, groups=groups, n_groups=3)
    dev = eng.vpc(cs["sigma"], K, prior_mean=cs["prior_mean"], prior_sd=cs["prior_sd"], groups=groups, n_groups=3)
    nn1, cond1 = eng.get_params()
    assert np.array_equal(nn0, nn1) and np.array_equal(cond0, cond1)
    stream1 = eng.rng_draws(0, 2)
    assert np.array_equal(stream0[0], stream1[0]) and np.array_equal(stream0[1], stream1[1])
    assert np.array_equal(eng.mh_chain(None, None, 0.4, -0.6, 0.9, 0.3, n_mc=2)[1], chain0)       # the stream's position
    assert np.all(np.isfinite(dev["simulated_ci"]))
    neg = cs["sigma"].copy()
    neg[9] = -1e-3
    over = groups.copy()
    over[12] = 3
    kw = dict(noise=noise, groups=groups, n_groups=3)
    bad_calls = [
        lambda: eng.vpc(cs["sigma"], 1, cond[:1], noise=noise[:1], groups=groups, n_groups=3),      # n_sims = 1
        lambda: eng.vpc(cs["sigma"], 4097, np.zeros((4097, N))),                                    # n_sims = 4097
        lambda: eng.vpc(cs["sigma"], K, cond, first_rep=-1, **kw),
        lambda: eng.vpc(cs["sigma"], K, cond, first_rep=2 ** 47 - K + 1, **kw),
        lambda: eng.vpc(cs["sigma"], K, cond, state=1, **kw),                                       # c-peptide: the observed state only
        lambda: eng.vpc(neg, K, cond, **kw),                                                        # a negative sigma
        lambda: eng.vpc(cs["sigma"], K, prior_sd=0.0),                                              # no cond_sets: prior_sd > 0
        lambda: eng.vpc(cs["sigma"], K, prior_sd=float("nan")),
        lambda: eng.vpc(cs["sigma"], K, cond, noise=noise, groups=over, n_groups=3),                # an id >= n_groups
        lambda: eng.vpc(cs["sigma"], K, cond, noise=noise, groups=groups, n_groups=9),
        lambda: eng.vpc(cs["sigma"], K, cond, noise=noise, groups=groups, n_groups=0),
        lambda: eng.vpc(cs["sigma"], K, cond, levels=(0.5, 0.5), **kw),                             # not strictly increasing
        lambda: eng.vpc(cs["sigma"], K, cond, levels=(0.1, 1.5), **kw),
        lambda: eng.vpc(cs["sigma"], K, cond, levels=np.linspace(0.1, 0.9, 9), **kw),               # nine levels
        lambda: eng.vpc(cs["sigma"], K, cond, levels=(), **kw),
        lambda: eng.vpc(cs["sigma"], K, cond, ci_levels=(0.9, 0.1), **kw),
        lambda: eng.vpc(cs["sigma"], K, cond, ci_levels=(-0.1, 0.5), **kw),
        lambda: eng.vpc(cs["sigma"], K, cond, ci_levels=np.linspace(0.1, 0.9, 9), **kw),
    ]
    for n, call in enumerate(bad_calls):
        with pytest.raises(CudeError) as e:
            call()
        assert e.value.status == -1, (n, e.value)                                                   # CUDE_ERR_ARG
    # outputs: none of the first three is an error, any one of them is enough; the counts and the status are optional
    sg, lv, cv = np.ascontiguousarray(cs["sigma"]), np.array(LEVELS), np.array(CI)

    def raw(obs_q, sim_ci, sim_q, n_mem=None, n_used=None, status=None, sigma=sg):
        return eng._lib.cude_vpc(eng._h, K, _ptr(cond), 0.0, 1.0, _ptr(sigma), 0, _ptr(noise), 0, 3, _ptr(groups), 3, _ptr(lv), 3,
                                 _ptr(cv), _ptr(obs_q), _ptr(sim_ci), _ptr(sim_q), _ptr(n_mem), _ptr(n_used), _ptr(status))
    n_mem, st = np.empty(3, dtype=np.int32), np.empty(N, dtype=np.int32)
    assert raw(None, None, None, n_mem, None, st) == -1
    obs_q, sim_ci, sim_q = np.empty((3, R, 3)), np.empty((3, R, 3, 3)), np.empty((K, 3, R, 3))
    assert raw(obs_q, None, None, sigma=None) == -1
    assert raw(obs_q, None, None) == 0 and vr.same(obs_q, full["observed"])
    assert raw(None, sim_ci, None) == 0 and vr.same(sim_ci, full["simulated_ci"])
    assert raw(None, None, sim_q, n_mem, None, st) == 0 and vr.same(sim_q, full["simulated_q"])
    assert np.array_equal(n_mem, full["n_members"]) and np.array_equal(st, full["status"])
    # groups = None: everybody in group 0; prior_sd is not looked at when cond_sets is given
    one = eng.vpc(cs["sigma"], K, cond, noise=noise, prior_sd=0.0)
    assert one["n_members"][0] == N and np.all(one["status"] == 0)
    assert vr.same(one["observed"], eng.vpc(cs["sigma"], K, cond, noise=noise, groups=np.zeros(N, dtype=np.int32))["observed"])
    eng.close()
    sup = vr.case("supp-4355", 67)
    eng = vr.make_engine(sup)
    with pytest.raises(CudeError) as e:
        eng.vpc(sup["sigma"], K, vr.draws(sup, K)[0], state=3)
    assert e.value.status == -1
    eng.close()
    # call order
    eng = Engine("cpep", cs["arch"], n_steps=cs["n_steps"], n_state=cs["n_state"])
    with pytest.raises(CudeError) as e:
        eng.N, eng.T = N, cs["T"]
        eng.vpc(cs["sigma"], K, cond)
    assert e.value.status == -3                                                                     # no population
    eng.set_population_cpep(cs["tp"], cs["G"], cs["obs"], cs["age"], cs["t2dm"])
    with pytest.raises(CudeError) as e:
        eng.vpc(cs["sigma"], K, cond)
    assert e.value.status == -3                                                                     # no shared parameters
    eng.close()
    # the fallback kernel
    eng = Engine("cpep", cs["arch"], n_steps=cs["n_steps"], n_state=cs["n_state"])
    eng.set_option("force_fallback", 1)
    eng.set_network([cs["arch"][1]] * cs["arch"][2], ["tanh"] * cs["arch"][2] + ["softplus"])
    assert eng.fallback_kernel
    eng.set_population_cpep(cs["tp"], cs["G"], cs["obs"], cs["age"], cs["t2dm"])
    eng.set_params(cs["nn"], None)
    with pytest.raises(CudeError) as e:
        eng.vpc(cs["sigma"], K, cond)
    assert e.value.status == -4 and "fallback" in str(e.value)                                      # CUDE_ERR_UNSUPPORTED
    eng.close()


# ----------------------------------------------------------------------------- 10. the mirrors
def test_api_vpc_reproduces_the_calibration_study(fixed_step_default):
    """tests/test_vpc_host.py's two cases through api.vpc: `outside` is what the restatement gives on the device's own
    simulated observations, and it says what the CPU study says -- at most 2 of the 15 cells for the data drawn from the
    model, the median of every row for the data drawn 3 prior_sd off."""
    from cude import api
    net = api.chain(4, 2, input_dims=2)
    for shift in (0.0, 3.0):
        cs = vr.case("cpep-2441", vr.N_CAL, data_seed=vr.CAL_DATA_SEED, obs_shift=shift)
        cond, noise = vr.draws(cs, vr.K_CAL, seed=29)
        models = [api.CPeptideConditionalUDEModel(cs["G"][i], cs["tp"], cs["age"][i], net, cs["obs"][i], bool(cs["t2dm"][i]))
                  for i in range(vr.N_CAL)]
        r = api.vpc(cs["nn"], models, cs["tp"], cs["obs"], cs["sigma"], cs["prior_mean"], cs["prior_sd"], n_sims=vr.K_CAL,
                    samples=cond, noise=noise, n_steps=cs["n_steps"])
        eng = vr.make_engine(cs)
        sims = eng.npde(cs["sigma"], vr.K_CAL, cond, noise=noise, want_sims=True, want_decorrelated=False)["sims"]
        eng.close()
        ref = vr.vpc(sims, cs["y_obs"], cs["sigma"], None, 1, LEVELS, CI)
        assert vr.same(r.observed, ref["observed"]) and vr.same(r.simulated_ci, ref["simulated_ci"])
        assert np.array_equal(r.outside, ref["outside"]) and r.outside.shape == (1, cs["R"], 3) and r.labels is None
        assert np.array_equal(r.levels, LEVELS) and np.array_equal(r.ci_levels, CI)
        assert list(r.n_members) == [vr.N_CAL] and list(r.n_sims_used) == [vr.K_CAL] and np.all(r.status == 0)
        print(f"api.vpc, shift {shift}: {np.count_nonzero(r.outside)} of {r.outside.size} cells outside")
        if shift == 0.0:
            assert np.count_nonzero(r.outside) <= 2
        else:
            assert np.all(r.outside[0, :, 1])
        # strata by label, in order of first appearance
        names = np.where(cs["t2dm"] > 0, "T2DM", np.where(np.arange(vr.N_CAL) % 2 == 0, "NGT", "IGT"))
        s = api.vpc(cs["nn"], models, cs["tp"], cs["obs"], cs["sigma"], cs["prior_mean"], cs["prior_sd"], groups=list(names),
                    n_sims=vr.K_CAL, samples=cond, noise=noise, n_steps=cs["n_steps"])
        assert sorted(s.labels) == sorted(set(names)) and s.labels[0] == names[0]
        ids = np.array([s.labels.index(v) for v in names])
        ref = vr.vpc(sims, cs["y_obs"], cs["sigma"], ids, len(s.labels), LEVELS, CI)
        assert vr.same(s.observed, ref["observed"]) and vr.same(s.simulated_ci, ref["simulated_ci"])
        assert np.array_equal(s.outside, ref["outside"]) and np.array_equal(s.n_members, np.bincount(ids))
    # the device stream, seeded: reproducible, another seed differs
    kw = dict(n_sims=50, n_steps=cs["n_steps"])
    d1 = api.vpc(cs["nn"], models, cs["tp"], cs["obs"], cs["sigma"], cs["prior_mean"], cs["prior_sd"], seed=5, **kw)
    d2 = api.vpc(cs["nn"], models, cs["tp"], cs["obs"], cs["sigma"], cs["prior_mean"], cs["prior_sd"], seed=5, **kw)
    d3 = api.vpc(cs["nn"], models, cs["tp"], cs["obs"], cs["sigma"], cs["prior_mean"], cs["prior_sd"], seed=6, **kw)
    assert np.array_equal(d1.simulated_ci, d2.simulated_ci) and not np.array_equal(d1.simulated_ci, d3.simulated_ci)
    api.clear_cache()


def test_api_suppression_vpc_end_to_end(fixed_step_default):
    from cude import api
    cs = vr.case("supp-4355", 67)
    K, groups = 64, _groups67()
    cond, noise = vr.draws(cs, K)
    prob = api.SuppressionProblem(api.chain(3, 5, input_dims=4))
    p = api.ComponentArray(theta=np.zeros(cs["N"]), neural=cs["nn"])
    r = api.suppression_vpc(p, (prob, cs["data"], cs["tp"], 0.0), cs["sigma"], cs["prior_mean"], cs["prior_sd"],
                            state=cs["state"], groups=groups, n_sims=K, samples=cond, noise=noise, n_steps=cs["n_steps"])
    eng = vr.make_engine(cs)
    want = eng.vpc(cs["sigma"], K, cond, noise=noise, state=cs["state"], groups=groups, n_groups=3)
    eng.close()
    assert vr.same(r.observed, want["observed"]) and vr.same(r.simulated_ci, want["simulated_ci"])
    assert np.array_equal(r.n_members, want["n_members"]) and np.array_equal(r.status, want["status"])
    assert np.array_equal(r.outside, (want["observed"] < want["simulated_ci"][..., 0]) | (want["observed"] > want["simulated_ci"][..., -1]))
    api.clear_cache()
