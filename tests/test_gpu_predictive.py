"""cude_predictive_bands and cude_evaluate_conditional_sets on the device against the rules restated in numpy
(tests/predictive_ref.py), driven by the device's OWN per-set solves: v[k] = eng.simulate(times) after
set_params(None, cond_sets[k]) for the bands, np.diagonal(eng.profile_conditional(cond_sets[k])) for the SSEs.

Bar: exact equality.  The bands are selections among those values and one sum in a fixed order, the best set is an exact
minimum with the lowest index, so nothing is left for a tolerance to absorb -- whatever the split of the solves over
subjects ("predictive_subjects") and output times ("predictive_times") and of the sets over launches ("profile_chunk").

Shapes: N = 70 (one full wave and six lanes) and N = 5; K = 1, 2, 37 (padding of the sort live) and 130 (more than two
waves of lanes, tile of 32 columns); 11 output times with both ends of the span, the data times and a repeated time.
The adaptive c-peptide solve has two states (the cumulative third one exists in fixed-step mode only): state 0 there."""
import numpy as np
import pytest
import torch  # noqa: F401  (first: shared HIP runtime)

from conftest import make_cpep_case, make_supp_case
import predictive_ref as pr

pytestmark = pytest.mark.gpu

KS = (1, 2, 37, 130)
PEN = (0.35, -0.6)
SYM_P0, SYM_STEPS = 1.78, 32

# name -> (model, arch, states checked in fixed-step mode, in adaptive mode)
CASES = {
    "cpep-2441": ("cpep", (2, 4, 2), (2,), (0,)),
    "cpep-2661": ("cpep", (2, 6, 2), (2,), (0,)),
    "supp-4355": ("supp", (4, 3, 5), (1, 2), (1, 2)),
    "sym-raw": ("cpep_sym", (1, 0, 0), (2,), (0,)),
}
_DATA = {}


def _case(model, arch, N):
    key = (model, arch, N)
    if key not in _DATA:
        if model == "supp":
            _DATA[key] = make_supp_case(N, arch)
        elif model == "cpep_sym":
            c = make_cpep_case(N, (2, 4, 2))
            _DATA[key] = dict(c, nn=np.array([SYM_P0]), beta=np.full(N, 20.0))
        else:
            _DATA[key] = make_cpep_case(N, arch)
    return _DATA[key]


def _make(name, n_steps, N, fallback=False):
    """(engine with parameters set, its conditional parameters)"""
    from cude.engine import Engine
    model, arch, _, _ = CASES[name]
    c = _case(model, arch, N)
    if model == "supp":
        eng = Engine("supp", arch, n_steps=n_steps)
        eng.set_population_supp(c["tp"], c["data"])
        cond = c["theta"]
    else:
        steps = n_steps if (model == "cpep" or n_steps == 0) else SYM_STEPS
        eng = Engine(model, arch, n_steps=steps, n_state=2 if n_steps == 0 else 3,
                     cond_space="raw" if model == "cpep_sym" else "log")
        if fallback:
            eng.set_option("force_fallback", 1)
            eng.set_network([arch[1]] * arch[2], ["tanh"] * arch[2] + ["softplus"])
            assert eng.fallback_kernel
        eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
        cond = c["beta"]
    eng.set_params(c["nn"], cond)
    return eng, np.array(cond, dtype=np.float64), np.asarray(c["tp"], dtype=np.float64)


def _times(tp):
    """11 non-decreasing output times: the data times (both ends of the span among them), times between them, one of them twice"""
    frac = np.array([0.07, 0.19, 0.31, 0.43, 0.57, 0.71, 0.83, 0.93])
    keep = np.unique(np.concatenate([tp, tp[0] + (tp[-1] - tp[0]) * frac[: max(0, 10 - tp.size)]]))
    assert keep.size == 10, (tp.size, keep.size)
    t = np.sort(np.concatenate([keep, keep[4:5]]))
    assert t.size == 11 and t[0] == tp[0] and t[-1] == tp[-1]
    return t


def _samples(cond, K, seed=4):
    return cond[None, :] + 0.4 * np.random.default_rng(seed).standard_normal((K, cond.size))


def _per_set(eng, cond, sets, times):
    """v (K, n_state, n_times, N): the device's own solves, one set at a time; the context's parameters restored"""
    v = []
    for row in sets:
        eng.set_params(None, row)
        v.append(eng.simulate(times))
    eng.set_params(None, cond)
    return np.stack(v)


def _ranks(K):
    return np.unique([0, min(1, K - 1), K // 2, max(K - 2, 0), K - 1]).astype(np.int32)


def _same(tag, got, want):
    for k in ("order", "mean", "bad_sets"):
        if want[k] is None or got[k] is None:
            assert want[k] is None and got[k] is None or k != "bad_sets", (tag, k)
            continue
        same = np.array_equal(got[k], want[k], equal_nan=True)
        if not same:
            g, w = np.asarray(got[k], dtype=float), np.asarray(want[k], dtype=float)
            bad = np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))
            print(f"{tag}: {k} differs at {bad[:6].tolist()}: device {g[tuple(bad[:6].T)]} restatement {w[tuple(bad[:6].T)]}")
        assert same, (tag, k)


@pytest.mark.parametrize("N", [70, 5])
@pytest.mark.parametrize("n_steps", [30, 0], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("name", list(CASES))
def test_bands_equal_the_restatement(name, n_steps, N):
    eng, cond, tp = _make(name, n_steps, N)
    times = _times(tp)
    sets = _samples(cond, max(KS))
    v = _per_set(eng, cond, sets, times)
    states = CASES[name][2 if n_steps else 3]
    for K in KS:
        for state in states:
            want = pr.bands(v[:K, state], _ranks(K))
            got = eng.predictive_bands(sets[:K], times, _ranks(K), state=state)
            print(f"{name} S={n_steps} N={N} K={K} state={state}: mean range {np.nanmin(want['mean']):.4g} .. {np.nanmax(want['mean']):.4g}")
            _same(f"{name} K={K} state={state}", got, want)
            assert eng.n_failed() == 0 and not got["bad_sets"].any()
            assert np.isfinite(got["order"]).all()
    assert np.array_equal(eng.get_params()[1], cond)            # the context's parameters are untouched
    if n_steps == 0:
        from cude._lib import CudeError
        with pytest.raises(CudeError):
            eng.adaptive_steps(0)
    eng.close()


@pytest.mark.parametrize("n_steps", [30, 0], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("name", ["cpep-2441", "supp-4355"])
def test_forced_splits_change_nothing(name, n_steps):
    eng, cond, tp = _make(name, n_steps, 70)
    times = _times(tp)
    K = 37
    sets = _samples(cond, K)
    state = CASES[name][2 if n_steps else 3][-1]
    whole = eng.predictive_bands(sets, times, _ranks(K), state=state)
    want = pr.bands(_per_set(eng, cond, sets, times)[:, state], _ranks(K))
    _same(name + " unsplit", whole, want)
    for subj, tms in ((64, 0), (0, 4), (64, 4), (1, 1)):       # two subject launches (the second partial), three time chunks
        eng.set_option("predictive_subjects", subj)
        eng.set_option("predictive_times", tms)
        _same(f"{name} split {subj}/{tms}", eng.predictive_bands(sets, times, _ranks(K), state=state), whole)
    eng.close()


@pytest.mark.parametrize("n_steps", [30, 0], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("name", ["cpep-2441", "supp-4355"])
def test_nan_sample_marks_its_subject_only(name, n_steps):
    eng, cond, tp = _make(name, n_steps, 70)
    times = _times(tp)
    K = 37
    sets = _samples(cond, K)
    state = 0 if name.startswith("cpep") else 2
    clean = eng.predictive_bands(sets, times, _ranks(K), state=state)
    sets[3, 7] = np.nan
    v = _per_set(eng, cond, sets, times)[:, state]
    nonfinite = ~np.isfinite(v[3, :, 7])
    print(f"{name} S={n_steps}: per-set simulate of the NaN sample is non-finite at output times {np.flatnonzero(nonfinite).tolist()}")
    assert np.isfinite(np.delete(v, 7, axis=2)).all()
    # Rule 4 is a test on the VALUES, and so is this one.  The c-peptide kernels' networks take the conditional parameter
    # through exp and the table-based tanh, which map a NaN to finite numbers: cude_simulate's trajectory of a NaN
    # conditional parameter is finite there (in either mode), so no column is marked.  The suppression solves carry
    # the NaN to every output.
    hit = int(nonfinite.any())
    assert hit == (0 if name.startswith("cpep") else 1)
    for subj, tms in ((0, 0), (64, 4)):
        eng.set_option("predictive_subjects", subj)
        eng.set_option("predictive_times", tms)
        got = eng.predictive_bands(sets, times, _ranks(K), state=state)
        _same(name + " NaN", got, pr.bands(v, _ranks(K)))
        assert np.array_equal(np.isnan(got["mean"][7]), nonfinite) and np.array_equal(np.isnan(got["order"][7]).all(axis=1), nonfinite)
        assert got["bad_sets"][7] == hit and got["bad_sets"].sum() == hit and eng.n_failed() == hit
        others = np.arange(70) != 7
        assert np.array_equal(got["order"][others], clean["order"][others])
        assert np.array_equal(got["mean"][others], clean["mean"][others])
    eng.close()


def test_outputs_that_can_be_omitted_and_errors():
    from cude._lib import CudeError
    eng, cond, tp = _make("cpep-2441", 30, 5)
    times = _times(tp)
    K = 37
    sets = _samples(cond, K)
    full = eng.predictive_bands(sets, times, _ranks(K), state=2)
    only_mean = eng.predictive_bands(sets, times, [], state=2)
    assert only_mean["order"] is None and np.array_equal(only_mean["mean"], full["mean"])
    only_order = eng.predictive_bands(sets, times, _ranks(K), state=2, want_mean=False)
    assert only_order["mean"] is None and np.array_equal(only_order["order"], full["order"])
    span = tp[-1] - tp[0]
    bad_calls = [
        lambda: eng.predictive_bands(sets[:0], times, [], state=2),                       # n_sets = 0
        lambda: eng.predictive_bands(np.zeros((4097, 5)), times, [0], state=2),           # n_sets = 4097
        lambda: eng.predictive_bands(sets, times, [0, K], state=2),                       # rank out of range
        lambda: eng.predictive_bands(sets, times, [-1, 3], state=2),
        lambda: eng.predictive_bands(sets, times, [3, 3], state=2),                       # not increasing
        lambda: eng.predictive_bands(sets, times, [5, 2], state=2),
        lambda: eng.predictive_bands(sets, times, np.arange(17), state=2),                # more than 16 ranks
        lambda: eng.predictive_bands(sets, np.append(times, tp[-1] + 0.01 * span), [0], state=2),     # outside the span
        lambda: eng.predictive_bands(sets, times[::-1], [0], state=2),
        lambda: eng.predictive_bands(sets, times, [0], state=3),                          # state = n_state
        lambda: eng.predictive_bands(sets, times, [], state=2, want_mean=False),          # no output
    ]
    for call in bad_calls:
        with pytest.raises(CudeError) as e:
            call()
        assert e.value.status == -1, e.value                                                 # CUDE_ERR_ARG
    eng.close()
    eng, cond, tp = _make("cpep-2441", 30, 5, fallback=True)
    with pytest.raises(CudeError) as e:
        eng.predictive_bands(_samples(cond, 3), _times(tp), [0], state=0)
    assert e.value.status == -4 and "fallback" in str(e.value)        # CUDE_ERR_UNSUPPORTED
    eng.close()


EV_CASES = [("cpep-2441", 24, False), ("cpep-2441", 70, False), ("supp-4355", 24, False), ("cpep-2441", 24, True)]


@pytest.mark.parametrize("n_steps", [30, 0], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("name,N,fallback", EV_CASES, ids=[f"{n}-{N}{'-fallback' if f else ''}" for n, N, f in EV_CASES])
def test_evaluate_conditional_sets(name, N, fallback, n_steps):
    eng, cond, tp = _make(name, n_steps, N, fallback)
    K = 37
    sets = _samples(cond, K, seed=9)
    sets[5] = sets[2]                                          # a duplicated set: the first one wins the tie
    sse = np.stack([np.diagonal(eng.profile_conditional(row)).copy() for row in sets])
    eng.set_option("profile_chunk", 8)                         # five launches, the last one partial
    for pw, pc in ((0.0, 0.0), PEN):
        got = eng.evaluate_conditional_sets(sets, pw, pc, want_sse=True)
        assert np.array_equal(got["sse"], sse)
        idx, best = pr.best_of_sets(sse, sets, pw, pc)
        print(f"{name} N={N} S={n_steps} pw={pw}: best sets {np.bincount(idx, minlength=K).tolist()}")
        assert np.array_equal(got["index"], idx) and np.array_equal(got["objective"], best)
        assert not np.any(got["index"] == 5)
    eng.set_option("profile_chunk", 0)
    again = eng.evaluate_conditional_sets(sets, *PEN)
    assert again["sse"] is None and np.array_equal(again["index"], idx) and np.array_equal(again["objective"], best)
    # a set of NaN never wins; a subject whose every value is NaN: index 0, +Inf
    sets[0] = np.nan
    sets[:, 3] = np.nan
    got = eng.evaluate_conditional_sets(sets, want_sse=True)
    idx, best = pr.best_of_sets(got["sse"], sets)
    assert np.array_equal(got["index"], idx) and np.array_equal(got["objective"], best)
    assert got["index"][3] == 0 and got["objective"][3] == np.inf and not np.any(got["index"][np.arange(N) != 3] == 0)
    assert np.array_equal(eng.get_params()[1], cond)
    eng.close()


def _api_models(api, c, arch, N):
    net = api.chain(arch[1], arch[2], "tanh")
    return [api.CPeptideConditionalUDEModel(c["G"][i], c["tp"], c["age"][i], net, c["obs"][i], bool(c["t2dm"][i]))
            for i in range(N)]


@pytest.mark.parametrize("n_steps", [30, 0], ids=["fixed", "adaptive"])
def test_posterior_predictive_mirror(n_steps):
    """quantiles against numpy.quantile over stacked api.simulate calls.  rtol 1e-14: the order statistics are the same
    bits, and either lerp makes at most three roundings of numbers no larger than the two neighbours, all positive."""
    from cude import api
    arch, N, K = (2, 4, 2), 24, 37
    c = make_cpep_case(N, arch)
    models = _api_models(api, c, arch, N)
    fine = np.round(np.arange(0.0, c["tp"][-1] + 1e-9, (c["tp"][-1] - c["tp"][0]) / 16), 10)
    sets = _samples(c["beta"], K)
    levels = (0.025, 0.5, 0.975, 0.0, 1.0)
    try:
        stack = np.stack([api.simulate(c["nn"], row, models, c["tp"], c["obs"], out_timepoints=fine, n_steps=n_steps)
                          for row in sets])                       # (K, N, n_times)
        pp = api.posterior_predictive(c["nn"], sets, models, c["tp"], c["obs"], out_timepoints=fine, levels=levels,
                                      n_steps=n_steps)
    finally:
        api.clear_cache()
    assert pp.quantiles.shape == (N, len(levels), fine.size) and pp.mean.shape == (N, fine.size)
    np.testing.assert_allclose(pp.quantiles, np.quantile(stack, levels, axis=0).transpose(1, 0, 2), rtol=1e-14, atol=0)
    assert np.array_equal(pp.minimum, stack.min(axis=0)) and np.array_equal(pp.maximum, stack.max(axis=0))
    assert np.array_equal(pp.mean, pr.sequential_mean(stack))
    assert not pp.bad_sets.any()


def test_suppression_predictive_mirror():
    from cude import api
    arch, N, K = (4, 3, 5), 16, 37
    c = make_supp_case(N, arch)
    prob = api.SuppressionProblem(api.chain(arch[1], arch[2], "tanh", input_dims=4))
    fine = np.linspace(0.0, 30.0, 13)
    sets = _samples(c["theta"], K)
    try:
        stack = np.stack([api.simul(api.ComponentArray(theta=row, neural=c["nn"]), prob, c["data"], fine, n_steps=30)
                          for row in sets])                       # (K, 3, n_times, N)
        pp = api.suppression_predictive(api.ComponentArray(theta=c["theta"], neural=c["nn"]), sets, prob, c["data"], fine,
                                        state=2, n_steps=30)
    finally:
        api.clear_cache()
    v = stack[:, 2].transpose(0, 2, 1)
    np.testing.assert_allclose(pp.quantiles, np.quantile(v, (0.025, 0.5, 0.975), axis=0).transpose(1, 0, 2), rtol=1e-14, atol=0)
    assert np.array_equal(pp.minimum, v.min(axis=0)) and np.array_equal(pp.maximum, v.max(axis=0))


def test_individual_effects_defaults_unchanged_and_sample_starts():
    """Default arguments: the same calls in the same order as before the new keywords existed (the chain, then the two
    penalised searches), so the same numbers from the same seed.  starts = "samples": refinement accepts decreasing
    objectives only and starts from the best kept sample, so it ends no worse than the search + 1e-9."""
    from cude import api
    arch, N = (2, 4, 2), 24
    c = make_cpep_case(N, arch)
    models = _api_models(api, c, arch, N)
    saem = api.SimpleNamespace(p_neural=c["nn"], eta=-0.6, Omega=0.9, sigma=0.4)
    n_samples = 90
    try:
        eff = api.individual_effects(models, c["tp"], c["obs"], saem, n_samples=n_samples, rng=np.random.default_rng(3),
                                     n_steps=30)
        # what the function did before it had the new keywords
        eng = api._population(models, c["tp"], c["obs"], 30).engine
        rng = np.random.default_rng(3)
        eng.set_params(c["nn"], np.full(N, -0.6))
        acc, samples = eng.mh_chain(rng.standard_normal((n_samples, N)), rng.random((n_samples, N)), 0.4, -0.6, 0.9, 0.3)
        pw = (0.4 / 0.9) ** 2
        modes, _, mse = eng.fit_conditional(-6.0, 4.0, 81, 48, pw, -0.6)
        mle, _, _ = eng.fit_conditional(-6.0, 4.0, 81, 48)
        assert np.array_equal(eff.samples, samples) and np.array_equal(eff.modes, modes)
        assert np.array_equal(eff.mle, mle) and np.array_equal(eff.mse, mse)
        assert eff.acceptance_rate == float(acc.sum()) / (n_samples * N) and not hasattr(eff, "predictive")

        fine = np.linspace(c["tp"][0], c["tp"][-1], 9)
        smp = api.individual_effects(models, c["tp"], c["obs"], saem, n_samples=n_samples, rng=np.random.default_rng(3),
                                     n_steps=30, starts="samples", predictive_times=fine)
        assert np.array_equal(smp.samples, samples)
        f_map = lambda x: eng.evaluate_conditional_sets(x[None, :], pw, -0.6)["objective"]
        f_mle = lambda x: eng.evaluate_conditional_sets(x[None, :])["objective"]
        print("MAP objective, samples - search:", np.max(f_map(smp.modes) - f_map(eff.modes)),
              " MLE:", np.max(f_mle(smp.mle) - f_mle(eff.mle)))
        assert np.all(f_map(smp.modes) <= f_map(eff.modes) + 1e-9)
        assert np.all(f_mle(smp.mle) <= f_mle(eff.mle) + 1e-9)
        kept = samples[n_samples // 3:][::10]
        assert smp.predictive.quantiles.shape == (N, 3, 9)
        want = pr.bands(np.stack([api.simulate(c["nn"], row, models, c["tp"], c["obs"], out_timepoints=fine, n_steps=30).T
                                  for row in kept]), [0, kept.shape[0] - 1])
        assert np.array_equal(smp.predictive.minimum, want["order"][:, :, 0])
        assert np.array_equal(smp.predictive.maximum, want["order"][:, :, 1])
        assert np.array_equal(smp.predictive.mean, want["mean"])
    finally:
        api.clear_cache()
