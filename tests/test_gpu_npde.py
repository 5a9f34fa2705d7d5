"""cude_npde on the device (csrc/cude_npde.hip): prediction discrepancies and npde per subject, against

  * cude_simulate set by set (rule 3) and rule 4 applied in numpy, to the bit;
  * the rules restated in numpy (tests/npde_ref.py), fed the device's own simulated observations;
  * itself: the subject split, device draws = their read-back fed in, a window of replicates, a shard of the subjects;
  * the calibration study of tests/test_npde_host.py through the api mirror.

Shapes: N = 70 (two solve workgroups, the second with six lanes; two reduce tiles), T = 6 (R = 5), n_steps 12 ... 30.

Bars of the reduction (the restatement forms every sum in the device's order, so most outputs are exact): n_used, below,
pred_mean and status equal; pred_var within 8 eps K relative (a sum of K rounded products and K rounded adds, divided
once); below_decorr equal outside the near-ties of the admission rule (npde_ref.near_ties: margin < 16 R^2 eps cond(C) (1 +
|w_obs|)), at most 1 % of a case's pairs (tests/test_npde_host.py counts them on the CPU oracle: none in any case); npde within
1e-14 max(1, |x|) of statistics.NormalDist().inv_cdf of the device's own counts (AS241 states 1e-16).

Not reachable from outside: CUDE_ERR_STATE under stream capture (the library captures inside cude_adam_run only)."""
from statistics import NormalDist

import numpy as np
import pytest
import torch  # noqa: F401

import npde_ref as nr

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
NONE = nr.SINGULAR | nr.FEW | nr.BAD_OBS


def _same(a, b, keys=None, subjects=None):
    for k in (keys or a):
        x, y = a[k], b[k]
        if subjects is not None:
            x, y = x[..., subjects], y[..., subjects]
        assert np.array_equal(x, y, equal_nan=(x.dtype.kind == "f")), k


def _check_reduction(label, got, cs_obs, sigma, K):
    """The device's outputs against the restatement applied to the device's own sims; returns the worst npde ratio."""
    ref = nr.reduce(got["sims"], cs_obs, sigma, want_aux=True)
    assert np.array_equal(got["n_used"], ref["n_used"]), label
    assert np.array_equal(got["status"], ref["status"]), label
    assert np.array_equal(got["below"], ref["below"]), label
    assert np.array_equal(got["pred_mean"], ref["pred_mean"], equal_nan=True), label
    assert np.array_equal(got["pd"], ref["pd"], equal_nan=True), label
    with np.errstate(invalid="ignore", divide="ignore"):
        dv = np.abs(got["pred_var"] - ref["pred_var"]) / np.abs(ref["pred_var"])
    assert np.array_equal(np.isnan(got["pred_var"]), np.isnan(ref["pred_var"])), label
    dv = dv[np.isfinite(dv)]
    ties, cond = nr.near_ties(ref)
    differ = got["below_decorr"] != ref["below_decorr"]
    print(f"{label}: pred_var {dv.max() / (EPS * K) if dv.size else 0.0:.2f} eps K; cond(C) up to {np.max(cond[np.isfinite(cond)], initial=0.0):.3g}; "
          f"near-ties {np.count_nonzero(ties)} of {ties.size}; below_decorr differs at {np.count_nonzero(differ)}")
    assert np.all(dv <= 8 * EPS * K), label
    assert np.count_nonzero(ties) <= 0.01 * ties.size, label
    assert not np.any(differ & ~ties), label
    # npde: the normal quantile of the device's own counts
    nd, worst = NormalDist(), 0.0
    none = (got["status"] & NONE) != 0
    assert np.all(got["below_decorr"][:, none] == -1) and np.all(np.isnan(got["npde"][:, none])), label
    for i in np.flatnonzero(~none):
        for r in range(got["npde"].shape[0]):
            x = nd.inv_cdf(nr.clipped(int(got["below_decorr"][r, i]), int(got["n_used"][i])))
            worst = max(worst, abs(got["npde"][r, i] - x) / (1e-14 * max(1.0, abs(x))))
    print(f"   npde vs inv_cdf: worst {worst:.3g} of the bar")
    assert worst <= 1.0, label
    return worst


# ----------------------------------------------------------------------------- 1. the solve and rule 4
@pytest.mark.parametrize("name", list(nr.CASES))
def test_sims_are_simulate_set_by_set_and_rule_4_to_the_bit(name):
    cs = nr.case(name)
    K, N, R = 5, cs["N"], cs["R"]
    cond, noise = nr.draws(cs, K)
    eng = nr.make_engine(cs)
    zero = eng.npde(np.zeros(N), K, cond, noise=noise, state=cs["state"], want_sims=True)
    v = np.empty((K, R, N))
    for k in range(K):
        eng.set_params(None, cond[k])
        v[k] = eng.simulate(cs["tp"])[cs["state"], 1:, :]
    assert np.array_equal(zero["sims"], v)
    # (sigma = 0: every simulation of a subject equal up to its conditional -- nothing here is asserted about the reduction)
    scale = 1.0 if cs["model"] != "supp" else eng.get_scale()[0][cs["state"]]
    got = eng.npde(cs["sigma"], K, cond, noise=noise, state=cs["state"], want_sims=True)
    assert np.array_equal(got["sims"], nr.observe(v, cs["sigma"], scale, noise))
    # the context's conditional parameters are the last set_params', untouched by the calls
    assert np.array_equal(eng.simulate(cs["tp"])[cs["state"], 1:, :], v[K - 1])
    eng.close()


# ----------------------------------------------------------------------------- 2. the reduction
@pytest.mark.parametrize("name", list(nr.CASES))
def test_reduction_follows_the_restatement_on_the_devices_own_sims(name):
    cs = nr.case(name)
    K = 65
    cond, noise = nr.draws(cs, K)
    eng = nr.make_engine(cs)
    got = eng.npde(cs["sigma"], K, cond, noise=noise, state=cs["state"], want_sims=True)
    assert eng.n_failed() == 0 and np.all(got["status"] == 0) and np.all(got["n_used"] == K)
    eng.close()
    _check_reduction(name, got, cs["y_obs"], cs["sigma"], K)
    # the device's solve against the CPU oracle's: the restatement of the whole call
    y = nr.observe(nr.solve_sets(cs, cond), cs["sigma"], cs["scale"], noise)
    assert np.max(np.abs(got["sims"] - y)) <= 1e-8 * np.max(np.abs(y))
    host = nr.reduce(y, cs["y_obs"], cs["sigma"])
    assert np.count_nonzero(got["below"] != host["below"]) <= 0.01 * host["below"].size
    assert np.max(np.abs(got["pred_mean"] - host["pred_mean"])) <= 1e-8 * np.max(np.abs(host["pred_mean"]))


@pytest.mark.parametrize("K", [2, 64, 65, 257, 1025, 4096])
def test_every_count_of_simulations_at_67_subjects(K):
    """N = 67: a full tile and one of three subjects; K walks the substitution's lanes (4 per subject at R = 5): fewer
    simulations than lanes, one round, one round and one, many rounds, the largest count.  K = 2 <= R: FEW."""
    cs = nr.case("cpep-2441", 67)
    cond, noise = nr.draws(cs, K)
    eng = nr.make_engine(cs)
    got = eng.npde(cs["sigma"], K, cond, noise=noise, want_sims=True)
    assert eng.n_failed() == (67 if K <= cs["R"] else 0)
    eng.close()
    assert np.all(got["status"] == (nr.FEW if K <= cs["R"] else 0))
    _check_reduction(f"K={K}", got, cs["y_obs"], cs["sigma"], K)


@pytest.mark.parametrize("T", [12, 32])
def test_more_rows_take_the_other_kernel_instances_and_a_narrower_tile(T):
    """R = 11: the substitution unrolled for 16 rows, 64 subjects per tile; R = 31, the most a population can have: unrolled
    for 31 rows, 14 subjects per tile (64 KiB of LDS) -- five tiles for 70 subjects, 18 lanes per subject."""
    cs = nr.case("supp-4355", T=T)
    K = 65
    cond, noise = nr.draws(cs, K)
    eng = nr.make_engine(cs)
    got = eng.npde(cs["sigma"], K, cond, noise=noise, state=cs["state"], want_sims=True)
    assert eng.n_failed() == 0 and np.all(got["status"] == 0)
    eng.set_option("npde_subjects", 64)
    _same(got, eng.npde(cs["sigma"], K, cond, noise=noise, state=cs["state"], want_sims=True))
    eng.close()
    _check_reduction(f"T={T}", got, cs["y_obs"], cs["sigma"], K)


# ----------------------------------------------------------------------------- 3. invariances
@pytest.mark.parametrize("name", ["cpep-2441", "supp-4355"])
def test_subject_split_gives_the_same_bits(name):
    cs = nr.case(name)
    K = 9
    cond, noise = nr.draws(cs, K)
    out = []
    for options in ((), (("npde_subjects", 64),)):
        eng = nr.make_engine(cs, options=options)
        out.append(eng.npde(cs["sigma"], K, cond, noise=noise, state=cs["state"], want_sims=True))
        out.append(eng.npde(cs["sigma"], K, state=cs["state"], want_sims=True, prior_mean=cs["prior_mean"],
                            prior_sd=cs["prior_sd"]))
        eng.close()
    _same(out[0], out[2])
    _same(out[1], out[3])
    assert np.unique(out[0]["sims"][:, :, 64:].reshape(-1, 6), axis=1).shape[1] == 6       # the last subjects are their own


def test_device_draws_are_their_read_back_and_depend_on_nothing_else():
    seed = 0x1234567890ABCDEF
    cs = nr.case("cpep-2441")
    N, R, K = cs["N"], cs["R"], 5
    eng = nr.make_engine(cs)
    eng.set_rng(seed)
    kw = dict(prior_mean=cs["prior_mean"], prior_sd=cs["prior_sd"], want_sims=True)
    a = eng.npde(cs["sigma"], K, **kw)
    z, eps = eng.npde_draws(0, K)
    assert z.shape == (K, N) and eps.shape == (K, R, N)
    # the counter layout of csrc/cude_rng.h (Box-Muller through libm here: a few ulp)
    for k, r, i in ((0, 0, 0), (4, R - 1, 69), (2, 3, 33)):
        zn, en = nr.eta_normal(seed, i, k), nr.noise_normal(seed, i, k, r)
        assert abs(z[k, i] - zn) <= 4e-15 * max(1.0, abs(zn)) and abs(eps[k, r, i] - en) <= 4e-15 * max(1.0, abs(en)), (k, r, i)
    assert 0.8 < z.std() < 1.2 and 0.8 < eps.std() < 1.2 and np.unique(np.concatenate([z.ravel(), eps.ravel()])).size == z.size + eps.size
    # rule 2's expression on the read-back, fed in as cond_sets / noise
    d = cs["prior_sd"] * z
    _same(a, eng.npde(cs["sigma"], K, cs["prior_mean"] + d, noise=eps, want_sims=True))
    # a window of the replicates: the caller's first_rep, no hidden position
    w = eng.npde(cs["sigma"], 2, first_rep=3, **kw)
    assert np.array_equal(w["sims"], a["sims"][3:5])
    z2, e2 = eng.npde_draws(3, 2)
    assert np.array_equal(z2, z[3:5]) and np.array_equal(e2, eps[3:5])
    # the Metropolis stream's position is untouched by all of this
    before = eng.rng_draws(0, 1)
    eng.close()
    # subjects 30 ... 69 in a context of their own
    sub = slice(30, 70)
    eng = nr.make_engine(cs, subjects=sub)
    eng.set_rng(seed, subject_offset=30)
    b = eng.npde(cs["sigma"][sub], K, **kw)
    assert np.array_equal(eng.rng_draws(0, 1)[0], before[0][:, sub])
    eng.close()
    for k in a:
        assert np.array_equal(a[k][..., sub], b[k], equal_nan=(a[k].dtype.kind == "f")), k


# ----------------------------------------------------------------------------- 4. status
def test_failed_simulations_leave_their_subject_only():
    """Suppression solves carry a NaN conditional parameter to every output (tests/test_gpu_predictive.py): the planned (k,
    i) fail, n_used drops by exactly those, and nobody else notices."""
    cs = nr.case("supp-4355")
    K = 12
    cond, noise = nr.draws(cs, K)
    eng = nr.make_engine(cs)
    kw = dict(noise=noise, state=cs["state"], want_sims=True)
    clean = eng.npde(cs["sigma"], K, cond, **kw)
    plan = [(0, 3), (5, 3), (11, 3), (7, 64), (2, 69)]
    bad = cond.copy()
    for k, i in plan:
        bad[k, i] = np.nan
    for options in ((), (("npde_subjects", 64),)):
        for k, v in options:
            eng.set_option(k, v)
        got = eng.npde(cs["sigma"], K, bad, **kw)
        assert eng.n_failed() == 0
        hit = np.zeros(cs["N"], dtype=int)
        for k, i in plan:
            hit[i] += 1
            assert np.all(np.isnan(got["sims"][k, :, i]))
        assert np.array_equal(got["n_used"], K - hit)
        assert np.array_equal(got["status"], np.where(hit > 0, nr.FAILED_SIMS, 0))
        _same(got, clean, subjects=np.flatnonzero(hit == 0))
        _check_reduction("failed sims", got, cs["y_obs"], cs["sigma"], K)
    eng.close()


def test_singular_few_and_bad_observations():
    cs = nr.case("cpep-2441")
    N, R, K = cs["N"], cs["R"], 12
    cond, noise = nr.draws(cs, K)
    eng = nr.make_engine(cs)
    clean = eng.npde(cs["sigma"], K, cond, noise=noise, want_sims=True)
    # one subject without residual noise and the same conditional parameter in every simulation: C = 0
    sigma, same = cs["sigma"].copy(), cond.copy()
    sigma[5] = 0.0
    same[:, 5] = cond[0, 5]
    got = eng.npde(sigma, K, same, noise=noise, want_sims=True)
    assert eng.n_failed() == 1 and got["status"][5] == nr.SINGULAR and np.all(np.delete(got["status"], 5) == 0)
    assert np.all(got["below_decorr"][:, 5] == -1) and np.all(np.isnan(got["npde"][:, 5]))
    y5 = got["sims"][:, :, 5]
    assert np.array_equal(got["below"][:, 5], np.sum(y5 < cs["y_obs"][None, :, 5], axis=0))
    assert np.array_equal(got["pd"][:, 5], [nr.clipped(int(b), K) for b in got["below"][:, 5]])
    _same(got, clean, subjects=np.delete(np.arange(N), 5))
    _check_reduction("singular", got, cs["y_obs"], sigma, K)
    # K = R: too few simulations for a factor of R rows
    few = eng.npde(cs["sigma"], R, cond[:R], noise=noise[:R], want_sims=True)
    assert eng.n_failed() == N and np.all(few["status"] == nr.FEW) and np.all(few["below_decorr"] == -1)
    assert np.all(np.isnan(few["npde"])) and np.all(np.isfinite(few["pd"])) and np.all(few["n_used"] == R)
    _check_reduction("few", few, cs["y_obs"], cs["sigma"], R)
    eng.close()
    # a NaN observation, a non-finite sigma
    obs = cs["obs"].copy()
    obs[68, 2] = np.nan
    eng = nr.make_engine(dict(cs, obs=obs))
    sg = cs["sigma"].copy()
    sg[1] = np.inf
    got = eng.npde(sg, K, cond, noise=noise, want_sims=True)
    assert eng.n_failed() == 2
    eng.close()
    for i in (1, 68):
        assert got["status"][i] == nr.BAD_OBS and got["n_used"][i] == -1
        assert np.all(got["below"][:, i] == -1) and np.all(got["below_decorr"][:, i] == -1)
        for k in ("pred_mean", "pred_var", "pd", "npde"):
            assert np.all(np.isnan(got[k][:, i])), k
    _same(got, clean, subjects=np.delete(np.arange(N), [1, 68]))


# ----------------------------------------------------------------------------- 5. adaptive mode
@pytest.mark.parametrize("name", ["cpep-2441", "supp-4355"])
def test_adaptive_mode(name):
    from cude._lib import CudeError
    cs = nr.case(name)
    K, N, R = 65, cs["N"], cs["R"]
    cond, noise = nr.draws(cs, K)
    eng = nr.make_engine(cs, n_steps=0)
    zero = eng.npde(np.zeros(N), K, cond, noise=noise, state=cs["state"], want_sims=True)
    for k in (0, 31, 64):
        eng.set_params(None, cond[k])
        assert np.array_equal(zero["sims"][k], eng.simulate(cs["tp"])[cs["state"], 1:, :]), k
    eng.loss_grad()
    eng.adaptive_steps(0)
    got = eng.npde(cs["sigma"], K, cond, noise=noise, state=cs["state"], want_sims=True)
    with pytest.raises(CudeError) as e:
        eng.adaptive_steps(0)
    assert e.value.status == -3
    scale = eng.get_scale()[0][cs["state"]] if cs["model"] == "supp" else 1.0
    eng.close()
    assert np.array_equal(got["sims"], nr.observe(zero["sims"], cs["sigma"], scale, noise))
    _check_reduction(name + " adaptive", got, cs["y_obs"], cs["sigma"], K)


# ----------------------------------------------------------------------------- 6. errors
def test_outputs_that_can_be_omitted_and_errors():
    from cude._lib import CudeError
    from cude.engine import Engine, _ptr
    cs = nr.case("cpep-2441")
    N, R, K = cs["N"], cs["R"], 8
    cond, noise = nr.draws(cs, K)
    eng = nr.make_engine(cs)
    full = eng.npde(cs["sigma"], K, cond, noise=noise)
    part = eng.npde(cs["sigma"], K, cond, noise=noise, want_decorrelated=False)
    assert "npde" not in part and np.array_equal(part["pd"], full["pd"]) and np.array_equal(part["status"], full["status"])
    neg = cs["sigma"].copy()
    neg[9] = -1e-3
    bad_calls = [
        lambda: eng.npde(cs["sigma"], 1, cond[:1], noise=noise[:1]),                      # n_sims = 1
        lambda: eng.npde(cs["sigma"], 4097, np.zeros((4097, N))),                         # n_sims = 4097
        lambda: eng.npde(cs["sigma"], K, cond, noise=noise, first_rep=-1),
        lambda: eng.npde(cs["sigma"], K, cond, noise=noise, first_rep=2 ** 47 - K + 1),
        lambda: eng.npde(cs["sigma"], K, cond, noise=noise, state=1),                     # c-peptide: the observed state only
        lambda: eng.npde(cs["sigma"], K, cond, noise=noise, state=-1),
        lambda: eng.npde(neg, K, cond, noise=noise),                                      # a negative sigma
        lambda: eng.npde(cs["sigma"], K, prior_sd=0.0),                                   # no cond_sets: prior_sd > 0
        lambda: eng.npde(cs["sigma"], K, prior_sd=float("nan")),
        lambda: eng.npde(cs["sigma"], K, prior_sd=-1.0),
        lambda: eng.npde_draws(0, 0),
        lambda: eng.npde_draws(2 ** 47, 1),
    ]
    for n, call in enumerate(bad_calls):
        with pytest.raises(CudeError) as e:
            call()
        assert e.value.status == -1, (n, e.value)                                         # CUDE_ERR_ARG
    # no output requested
    sg = np.ascontiguousarray(cs["sigma"])
    rc = eng._lib.cude_npde(eng._h, K, _ptr(cond), 0.0, 1.0, _ptr(sg), 0, _ptr(noise), 0, None, None, None, None, None, None,
                            None, None, None)
    assert rc == -1
    assert eng._lib.cude_npde_draws(eng._h, 0, K, None, None) == -1
    # prior_sd is not looked at when cond_sets is given
    assert np.array_equal(eng.npde(cs["sigma"], K, cond, noise=noise, prior_sd=0.0)["pd"], full["pd"])
    eng.close()
    sup = nr.case("supp-4355")
    eng = nr.make_engine(sup)
    with pytest.raises(CudeError) as e:
        eng.npde(sup["sigma"], K, nr.draws(sup, K)[0], state=3)
    assert e.value.status == -1
    eng.close()
    # call order
    eng = Engine("cpep", cs["arch"], n_steps=cs["n_steps"], n_state=cs["n_state"])
    with pytest.raises(CudeError) as e:
        eng.N, eng.T = N, cs["T"]
        eng.npde(cs["sigma"], K, cond)
    assert e.value.status == -3                                                            # no population
    eng.set_population_cpep(cs["tp"], cs["G"], cs["obs"], cs["age"], cs["t2dm"])
    with pytest.raises(CudeError) as e:
        eng.npde(cs["sigma"], K, cond)
    assert e.value.status == -3                                                            # no shared parameters
    eng.close()
    # the fallback kernel
    eng = Engine("cpep", cs["arch"], n_steps=cs["n_steps"], n_state=cs["n_state"])
    eng.set_option("force_fallback", 1)
    eng.set_network([cs["arch"][1]] * cs["arch"][2], ["tanh"] * cs["arch"][2] + ["softplus"])
    assert eng.fallback_kernel
    eng.set_population_cpep(cs["tp"], cs["G"], cs["obs"], cs["age"], cs["t2dm"])
    eng.set_params(cs["nn"], None)
    with pytest.raises(CudeError) as e:
        eng.npde(cs["sigma"], K, cond)
    assert e.value.status == -4 and "fallback" in str(e.value)                             # CUDE_ERR_UNSUPPORTED
    eng.close()


# ----------------------------------------------------------------------------- 7. the mirrors
def test_api_npde_reproduces_the_calibration_study(fixed_step_default):
    """tests/test_npde_host.py's study (70 subjects whose data are draws from the model, 500 simulations) through api.npde.
    The device's solves differ from the CPU oracle's by rounding, which moves a count only at a near-tie of y or w; the
    admission rule allows 1 % of the pairs, and one count more or less moves an npde by at most Phi^-1(2 / 1000) - Phi^-1(1 /
    1000) = 0.21 at K = 500 (the clip points, where the quantile is steepest).  Hence |d mean| <= 0.01 * 0.21 and, with |npde|
    <= 3.3, |d var| <= 0.01 * (2 * 3.3 * 0.21 + 0.21^2) (1 + 1 / n)."""
    from cude import api
    cs, cond, noise, host = nr.calibration()
    N = cs["N"]
    net = api.chain(4, 2, input_dims=2)
    models = [api.CPeptideConditionalUDEModel(cs["G"][i], cs["tp"], cs["age"][i], net, cs["obs"][i], bool(cs["t2dm"][i]))
              for i in range(N)]
    r = api.npde(cs["nn"], models, cs["tp"], cs["obs"], cs["sigma"], cs["prior_mean"], cs["prior_sd"], n_sims=nr.K_CAL,
                 samples=cond, noise=noise, n_steps=cs["n_steps"])
    want_mean, want_var = nr.pooled(host["npde"])
    print(f"api.npde: pooled mean {r.npde_mean:.6f} (host {want_mean:.6f}), variance {r.npde_var:.6f} (host {want_var:.6f})")
    assert (r.npde_mean, r.npde_var) == nr.pooled(r.npde)
    assert abs(r.npde_mean - want_mean) <= 0.01 * 0.21
    assert abs(r.npde_var - want_var) <= 0.01 * (2 * 3.3 * 0.21 + 0.21 ** 2) * (1 + 1 / r.npde.size)
    assert np.all(r.status == 0) and np.all(r.n_used == nr.K_CAL)
    assert np.count_nonzero(r.pd != host["pd"]) <= 0.01 * r.pd.size
    assert np.allclose(r.pred_sd, np.sqrt(host["pred_var"]), rtol=1e-7)
    # the device stream, seeded: reproducible, another seed differs; the shifted prior is seen
    kw = dict(n_sims=200, n_steps=cs["n_steps"])
    d1 = api.npde(cs["nn"], models, cs["tp"], cs["obs"], cs["sigma"], cs["prior_mean"], cs["prior_sd"], seed=5, **kw)
    d2 = api.npde(cs["nn"], models, cs["tp"], cs["obs"], cs["sigma"], cs["prior_mean"], cs["prior_sd"], seed=5, **kw)
    d3 = api.npde(cs["nn"], models, cs["tp"], cs["obs"], cs["sigma"], cs["prior_mean"], cs["prior_sd"], seed=6, **kw)
    d4 = api.npde(cs["nn"], models, cs["tp"], cs["obs"], cs["sigma"], cs["prior_mean"] + 2 * cs["prior_sd"], cs["prior_sd"],
                  seed=5, **kw)
    assert np.array_equal(d1.npde, d2.npde) and not np.array_equal(d1.npde, d3.npde)
    assert abs(d1.npde_mean) <= 4 / np.sqrt(d1.npde.size) < abs(d4.npde_mean)
    api.clear_cache()


def test_api_suppression_npde_end_to_end(fixed_step_default):
    from cude import api
    cs = nr.case("supp-4355")
    K = 64
    cond, noise = nr.draws(cs, K)
    prob = api.SuppressionProblem(api.chain(3, 5, input_dims=4))
    p = api.ComponentArray(theta=np.zeros(cs["N"]), neural=cs["nn"])
    r = api.suppression_npde(p, (prob, cs["data"], cs["tp"], 0.0), cs["sigma"], cs["prior_mean"], cs["prior_sd"],
                             state=cs["state"], n_sims=K, samples=cond, noise=noise, n_steps=cs["n_steps"])
    eng = nr.make_engine(cs)
    want = eng.npde(cs["sigma"], K, cond, noise=noise, state=cs["state"])
    eng.close()
    assert np.array_equal(r.npde, want["npde"]) and np.array_equal(r.pd, want["pd"])
    assert np.array_equal(r.pred_sd, np.sqrt(want["pred_var"])) and np.array_equal(r.n_used, want["n_used"])
    api.clear_cache()
