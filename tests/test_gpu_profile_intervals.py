"""cude_profile_intervals on the device against the rule restated in numpy (tests/profile_ref.py) and driven by the device's
OWN SSEs: the grid stage from eng.profile_conditional(values) and eng.forward at the centre, the rounds from an evaluator that
takes the diagonal of eng.profile_conditional(x) -- the same non-split kernel path the entry point launches.

Bar: exact equality of every output.  Every comparison of the rule is then made on identical bits on both sides, and every
reduction (minimum with the lowest index, min of `first`, max of `last`, sum of counts) is exact, so nothing is left for a
tolerance to absorb -- whatever the chunk size ("profile_chunk" = 8 on 37 points: five launches, the last one partial) and
however the set dimension is split over waves and workgroup rows (1000 points at N = 5).

Case settings (range, sigma, centre) were chosen on the CPU oracle so that closed, open, disconnected and below-centre
subjects all occur (tests/test_profile_intervals_host.py admits the flags); they are fixed here."""
import numpy as np
import pytest
import torch  # noqa: F401  (first: shared HIP runtime)

from conftest import make_cpep_case, make_supp_case
import profile_ref as pr

pytestmark = pytest.mark.gpu

DELTA95 = 7.16
PEN = (0.35, -0.6)
SYM_P0, SYM_STEPS = 1.78, 32
KEYS = ("lower", "upper", "argmin", "min", "center_objective", "n_inside", "status")

# name -> (model, arch, N, range of the scan, sigma, fallback kernel)
CASES = {
    "cpep-2441-24": ("cpep", (2, 4, 2), 24, (-4.0, 3.0), 0.1, False),
    "cpep-2441-70": ("cpep", (2, 4, 2), 70, (-4.0, 3.0), 0.1, False),
    "cpep-2661-24": ("cpep", (2, 6, 2), 24, (-4.0, 3.0), 0.1, False),
    "cpep-2661-70": ("cpep", (2, 6, 2), 70, (-4.0, 3.0), 0.1, False),
    "supp-4355-16": ("supp", (4, 3, 5), 16, (-6.0, 4.0), 0.3, False),
    "sym-raw-24": ("cpep_sym", (1, 0, 0), 24, (0.5, 400.0), 0.1, False),
    "cpep-2441-fallback": ("cpep", (2, 4, 2), 24, (-4.0, 3.0), 0.1, True),
}


def _sym_case(N, seed=20250905):
    """Observations the Michaelis-Menten production can follow: the oracle's solve of the symbolic model at
    k = 20 exp(beta) with 5 % multiplicative noise (as tests/test_gpu_refine.py's sym-raw case)."""
    import cude_oracle as o
    c = make_cpep_case(N, (2, 4, 2), seed=seed)
    pop = o.CPepPopulation(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"], covariate=False)
    traj = o.cpep_forward(np, np.array([SYM_P0]), 20.0 * np.exp(c["beta"]), pop, (1, 0, 0), SYM_STEPS, 2, "raw")
    u1 = np.stack([np.broadcast_to(np.asarray(traj[t][0], dtype=np.float64), (N,)) for t in range(len(c["tp"]))], axis=1)
    obs = u1 * (1.0 + 0.05 * np.random.default_rng(seed + 2).standard_normal(u1.shape))
    obs[:, 0] = c["obs"][:, 0]
    return dict(c, obs=obs, nn=np.array([SYM_P0]), beta=np.full(N, 20.0))


_DATA = {}


def _make(name, n_steps, N=None):
    """(engine with parameters set, the centres of the case)."""
    from cude.engine import Engine
    model, arch, n_def, box, sigma, fallback = CASES[name]
    N = n_def if N is None else N
    key = (model, arch, N)
    if key not in _DATA:
        _DATA[key] = make_supp_case(N, arch) if model == "supp" else (_sym_case(N) if model == "cpep_sym" else make_cpep_case(N, arch))
    c = _DATA[key]
    if model == "supp":
        eng = Engine("supp", arch, n_steps=n_steps)
        eng.set_population_supp(c["tp"], c["data"])
        center = c["theta"]
    else:
        steps = n_steps if (model == "cpep" or n_steps == 0) else SYM_STEPS
        eng = Engine(model, arch, n_steps=steps, cond_space="raw" if model == "cpep_sym" else "log")
        if fallback:
            eng.set_option("force_fallback", 1)
            eng.set_network([arch[1]] * arch[2], ["tanh"] * arch[2] + ["softplus"])
            assert eng.fallback_kernel
        eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
        center = c["beta"]
    eng.set_params(c["nn"], center)
    return eng, np.array(center, dtype=np.float64)


def _device_ev(eng):
    """SSE_i(x_i) through the scan's own launch: subject i's entry of the set that holds everybody at x_i."""
    return lambda x: np.diagonal(eng.profile_conditional(x)).copy()


def _center_sse(eng, center):
    eng.set_params(None, center)
    return eng.forward(want_sse=True)["sse"]


def _check(name, got, want):
    for k in KEYS:
        same = np.array_equal(got[k], want[k], equal_nan=True)
        if not same:
            bad = np.flatnonzero(~((got[k] == want[k]) | (np.isnan(got[k].astype(float)) & np.isnan(want[k].astype(float)))))
            print(f"{name}: {k} differs for subjects {bad[:8]}: device {got[k][bad[:8]]} restatement {want[k][bad[:8]]}")
        assert same, (name, k)


@pytest.mark.parametrize("n_steps", [30, 0], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("name", list(CASES))
def test_every_output_equals_the_restatement(name, n_steps):
    eng, center = _make(name, n_steps)
    model, arch, N, box, sigma, _ = CASES[name]
    values = np.linspace(box[0], box[1], 37)
    eng.set_option("profile_chunk", 8)                    # five launches, the last one partial
    prof = eng.profile_conditional(values)
    sse_c = _center_sse(eng, center)
    ev = _device_ev(eng)
    delta = 2 * sigma ** 2 * DELTA95
    # plain objective, one delta, centre = the context's conditional parameters, bisection and 3 sections
    for rounds, m in ((0, 3), (3, 3), (4, 1)):
        want = pr.intervals(ev, values, center, delta, rounds=rounds, sections=m, profile=prof, sse_center=sse_c)
        got = eng.profile_intervals(values, None, delta, rounds=rounds, sections=m)
        print(f"{name} S={n_steps} rounds={rounds} m={m}: status {dict(zip(*np.unique(want['status'], return_counts=True)))}, "
              f"closed ends {np.isfinite(want['lower']).sum()} + {np.isfinite(want['upper']).sum()}")
        _check(name, got, want)
        assert eng.n_failed() == 0
    assert np.isfinite(want["lower"]).sum() + np.isfinite(want["upper"]).sum() >= 4
    # penalised objective, one delta per subject, centres handed over, 16 sections
    pw, pc = (1e-4, 20.0) if model == "cpep_sym" else PEN
    dps = delta * np.linspace(0.5, 2.0, N)
    shifted = center + (0.05 if model != "cpep_sym" else 1.0)
    want = pr.intervals(ev, values, shifted, dps, pw, pc, rounds=2, sections=16, profile=prof,
                        sse_center=_center_sse(eng, shifted))
    got = eng.profile_intervals(values, shifted, delta_per_subject=dps, penalty_weight=pw, penalty_center=pc, rounds=2,
                                sections=16)
    _check(name + " penalised", got, want)
    # rule 6: minimum and argmin alone
    a = eng.profile_intervals(values, penalty_weight=pw, penalty_center=pc, argmin_only=True)
    assert np.array_equal(a["argmin"], want["argmin"]) and np.array_equal(a["min"], want["min"])
    # the chunk size changes nothing
    eng.set_option("profile_chunk", 0)
    again = eng.profile_intervals(values, shifted, delta_per_subject=dps, penalty_weight=pw, penalty_center=pc, rounds=2,
                                  sections=16)
    _check(name + " one chunk", again, got)
    if n_steps == 0:
        from cude._lib import CudeError
        with pytest.raises(CudeError):
            eng.adaptive_steps(0)                         # (the last solve was of a trial point)
    eng.close()


def test_set_dimension_split_over_waves_and_rows():
    """1000 points at N = 5: one launch of 1000 sets, reduced by 32 workgroup rows of 4 waves each."""
    eng, center = _make("cpep-2441-24", 30, N=5)
    values = np.linspace(-4.0, 3.0, 1000)
    prof = eng.profile_conditional(values)
    sse_c = _center_sse(eng, center)
    for pw, pc in ((0.0, 0.0), PEN):
        want = pr.intervals(_device_ev(eng), values, center, 2 * 0.1 ** 2 * DELTA95, pw, pc, rounds=2, sections=3,
                            profile=prof, sse_center=sse_c)
        got = eng.profile_intervals(values, None, 2 * 0.1 ** 2 * DELTA95, penalty_weight=pw, penalty_center=pc, rounds=2)
        _check("N=5 x 1000", got, want)
    eng.set_option("profile_chunk", 333)
    _check("N=5 x 1000 in chunks of 333", eng.profile_intervals(values, None, 2 * 0.1 ** 2 * DELTA95, penalty_weight=PEN[0],
                                                                penalty_center=PEN[1], rounds=2), want)
    eng.close()


def test_failed_centre_and_empty_interval():
    eng, center = _make("cpep-2441-24", 30)
    values = np.linspace(-4.0, 3.0, 37)
    bad = center.copy()
    bad[3] = np.nan
    bad[5] = 0.5 * (values[17] + values[18])              # off the grid: with a tiny delta nothing may lie inside
    prof = eng.profile_conditional(values)
    want = pr.intervals(_device_ev(eng), values, bad, 1e-9, rounds=2, profile=prof, sse_center=_center_sse(eng, bad))
    got = eng.profile_intervals(values, bad, 1e-9, rounds=2)
    _check("failed centre", got, want)
    assert got["status"][3] == pr.CENTER_FAILED and np.isnan(got["lower"][3]) and np.isnan(got["upper"][3])
    assert got["center_objective"][3] == np.inf and got["n_inside"][3] == 0 and eng.n_failed() == 1
    assert np.any(got["status"] & pr.EMPTY)
    # +Inf is a legal delta: everything finite lies inside, both ends open
    r = eng.profile_intervals(values, center, np.inf)
    assert np.all(r["status"] & 3 == 3) and np.all(r["n_inside"] == 37) and np.all(r["lower"] == -np.inf)
    eng.close()


def test_argument_errors_return_their_status():
    from cude._lib import CudeError
    from cude.engine import Engine
    eng, center = _make("supp-4355-16", 30)
    values = np.linspace(-6.0, 4.0, 9)

    def status_of(*a, **k):
        with pytest.raises(CudeError) as e:
            eng.profile_intervals(*a, **k)
        return e.value.status
    ARG, STATE = -1, -3
    probe = Engine("supp", (4, 3, 5), n_steps=30)
    with pytest.raises(CudeError) as e:
        probe.profile_intervals(values, None, 1.0)        # no population yet
    assert e.value.status == STATE
    probe.close()
    assert status_of(values[::-1].copy(), center, 1.0) == ARG
    assert status_of(np.r_[values[:4], values[3], values[5:]], center, 1.0) == ARG          # not strictly increasing
    assert status_of(np.r_[values[:4], np.inf], center, 1.0) == ARG
    assert status_of(values[:1], center, 1.0) == ARG
    assert status_of(values, center, 1.0, sections=0) == ARG and status_of(values, center, 1.0, sections=17) == ARG
    assert status_of(values, center, 1.0, rounds=-1) == ARG
    assert status_of(values, center, -1.0) == ARG and status_of(values, center, np.nan) == ARG
    assert status_of(values, center, delta_per_subject=np.r_[np.ones(15), -1.0]) == ARG
    assert status_of(values, center, delta_per_subject=np.r_[np.ones(15), np.nan]) == ARG
    r = eng.profile_intervals(values, center, 1.0)        # and the context still works
    assert r["status"].shape == (16,)
    eng.close()


# ----------------------------------------------------------------------------- the mirrors
@pytest.mark.parametrize("per_subject", [False, True], ids=["sigma", "sigma-per-subject"])
def test_api_equals_the_host_path(per_subject):
    """api.profile_confidence_intervals(rounds = 0) is find_confidence_intervals on every row of likelihood_profiles."""
    from cude import api
    N = 24
    c = make_cpep_case(N, (2, 4, 2))
    net = api.chain(4, 2, "tanh")
    models = [api.CPeptideConditionalUDEModel(c["G"][i], c["tp"], c["age"][i], net, c["obs"][i], bool(c["t2dm"][i]))
              for i in range(N)]
    sigma = np.linspace(0.05, 0.3, N) if per_subject else 0.1
    for n_steps in (30, None):
        nll, nll_min, values = api.likelihood_profiles(c["beta"], c["nn"], models, c["tp"], c["obs"], -4.0, 3.0, 1.0,
                                                       steps=200, n_steps=n_steps)          # sigma = 1: SSE / 2
        for target in ("cantelli95", "cantelli90", "raue95", "something-else"):
            cis, det = api.profile_confidence_intervals(c["beta"], c["nn"], models, c["tp"], c["obs"], -4.0, 3.0, sigma,
                                                        steps=200, target=target, n_steps=n_steps, return_details=True)
            assert len(cis) == N
            for i in range(N):
                s2 = (sigma[i] if per_subject else sigma) ** 2
                try:
                    want = api.find_confidence_intervals(nll[i] / s2, nll_min[i] / s2, values, target=target)
                except ValueError:
                    want = (np.nan, np.nan)
                    assert det["status"][i] & pr.EMPTY
                assert np.array_equal(np.array(cis[i]), np.array(want), equal_nan=True), (target, i, cis[i], want)
        # ten rounds of three sections: every closed end within one grid spacing inside the grid's answer
        fine = api.profile_confidence_intervals(c["beta"], c["nn"], models, c["tp"], c["obs"], -4.0, 3.0, sigma, steps=200,
                                                target="cantelli95", rounds=10, sections=3, n_steps=n_steps)
        grid = api.profile_confidence_intervals(c["beta"], c["nn"], models, c["tp"], c["obs"], -4.0, 3.0, sigma, steps=200,
                                                target="cantelli95", n_steps=n_steps)
        h, closed = values[1] - values[0], 0
        for (flo, fhi), (glo, ghi) in zip(fine, grid):
            if np.isfinite(glo):
                assert glo - h < flo <= glo
                closed += 1
            else:
                assert np.array_equal(flo, glo, equal_nan=True)
            if np.isfinite(ghi):
                assert ghi <= fhi < ghi + h
                closed += 1
            else:
                assert np.array_equal(fhi, ghi, equal_nan=True)
        assert closed >= N // 2
    api.clear_cache()


def test_api_suppression_and_symbolic_models():
    from cude import api
    c = make_supp_case(16)
    prob = api.SuppressionProblem(api.chain(3, 5, "tanh", input_dims=4))
    p = api.ComponentArray(theta=c["theta"], neural=c["nn"])
    cis, det = api.suppression_profile_intervals(p, (prob, c["data"], c["tp"], 0.0), -6.0, 4.0, 0.3, steps=37, rounds=3,
                                                 n_steps=30, return_details=True)
    from cude.engine import Engine
    eng = Engine("supp", c["arch"], n_steps=30)
    eng.set_population_supp(c["tp"], c["data"])
    eng.set_params(c["nn"], c["theta"])
    want = eng.profile_intervals(np.linspace(-6.0, 4.0, 37), None, 2 * 0.3 ** 2 * DELTA95, rounds=3)
    eng.close()
    assert np.array_equal(np.array(cis), np.stack([want["lower"], want["upper"]], axis=1), equal_nan=True)
    assert np.array_equal(det["status"], want["status"])
    # a list of CPeptideODEModel profiles the raw k
    s = _sym_case(24)
    models = [api.CPeptideODEModel(s["G"][i], s["tp"], s["age"][i], api.production, s["obs"][i], bool(s["t2dm"][i]))
              for i in range(24)]
    cis = api.profile_confidence_intervals(s["beta"], None, models, s["tp"], s["obs"], 0.5, 400.0, 0.1, steps=37, rounds=2,
                                           sections=1, n_steps=SYM_STEPS)
    eng, center = _make("sym-raw-24", 30)
    want = eng.profile_intervals(np.linspace(0.5, 400.0, 37), None, 2 * 0.1 ** 2 * DELTA95, rounds=2, sections=1)
    eng.close()
    assert np.array_equal(np.array(cis), np.stack([want["lower"], want["upper"]], axis=1), equal_nan=True)
    assert np.isfinite(np.array(cis)).sum() >= 8
    api.clear_cache()
