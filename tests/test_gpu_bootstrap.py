"""cude_bootstrap_conditional on the device (csrc/cude_bootstrap.hip, the replicate family of csrc/cude_refine.hip): the
parametric bootstrap of the per-subject fits, against

  * the rules restated in numpy (tests/bootstrap_ref.py) on the cases tests/test_bootstrap_host.py admits, fed the device's
    own prediction so that both sides fit the same replicate data bit for bit;
  * itself: every chunking and the subject split, host noise = device draws read back, a window of replicates, a shard of
    the subjects, the stepped form, a failed subject's neighbours.

Bars: tests/test_gpu_refine.py's.  |x - x_ref| <= 1e-6 (1 + |x|) at xtol = 1e-7 for every pair; statuses equal except for
the pairs the restatement itself decides differently under the tangent kernels' accepted error (bootstrap_ref.unstable_pairs,
at most 2 % of a case's pairs: tests/test_bootstrap_host.py) -- `evals` are not reported by this entry point.  Summaries:
n_used equal; an order statistic and the mean inherit the x bar (a selection / an average of values inside it); the sd, a
norm of the centred vector, moves by at most sqrt(n / (n - 1)) times the largest |dx|.  Against the restatement applied to
the device's own replicates the order statistics and n_used are exact, mean and sd agree to rounding (1e-13).

Not reachable from outside: CUDE_ERR_STATE under stream capture (the library captures inside cude_adam_run only)."""
import numpy as np
import pytest
import torch  # noqa: F401

pytestmark = pytest.mark.gpu

X_BAR = 1e-6
RANKS = [0, 3, 7]


def _make(name, N=None, n_steps=30, options=()):
    import test_gpu_refine as tg
    c, eng, _ = tg._make(name, N, n_steps)
    for k, v in options:
        eng.set_option(k, v)
    return c, eng, tg.CASES[name]


def _yhat(eng, center, supp):
    eng.set_params(None, center)
    traj = eng.forward(want_traj=True)["traj"]              # (n_state, T, N)
    return np.ascontiguousarray(traj if supp else traj[:1])


def _same(a, b, keys=None):
    for k in (keys or a):
        if a[k] is None:
            assert b[k] is None, k
        else:
            assert np.array_equal(a[k], b[k], equal_nan=True), k


def _cpep_inputs(N, B, seed=11):
    """(case data, centre, sigma, noise (B, T, N)) of the 2-4-4-1 population: a smooth spread of centres, 5 % noise."""
    import test_gpu_refine as tg
    c = tg._case_data("cpep-2441", N)
    rng = np.random.default_rng(seed)
    return c, np.linspace(-1.5, 0.5, N), np.full(N, 0.05), rng.standard_normal((B, len(c["tp"]), N))


# ----------------------------------------------------------------------------- 1. fused form vs the restatement
@pytest.mark.parametrize("name", ["cpep-2441", "supp-4355", "cpep-3441", "sym-raw"])
def test_fused_form_follows_the_restatement(name):
    import bootstrap_ref as br
    host = br.case(name)                                     # centre, sigma and noise of the admitted case
    c, eng, spec = _make(name, options=(("bootstrap_chunk", 3),))       # chunks of 3, 3 and 2 replicates
    supp = spec[0] == "supp"
    cs = br.case(name, yhat=_yhat(eng, host["center"], supp), center=host["center"], sigma=host["sigma"])
    assert np.max(np.abs(cs["yhat"] - host["yhat"])) <= 1e-9 * np.max(np.abs(host["yhat"]))
    B, N, box = cs["B"], cs["N"], cs["box"]
    want = br.refit(cs["make_ev"](), cs["center"], B, *box, **cs["kw"])
    got = eng.bootstrap_conditional(cs["sigma"], B, cs["center"], ranks=RANKS, noise=cs["noise"], lower=box[0], upper=box[1],
                                    max_step=cs["kw"]["max_step"], want_replicates=True)
    eng.close()
    dx = np.abs(got["replicates"] - want["x"]) / (1 + np.abs(want["x"]))
    differ = got["status"] != want["status"]
    print(f"{name}: max |dx|/(1+|x|) {dx.max():.2e}; status ref {np.bincount(want['status'].ravel(), minlength=5)} dev "
          f"{np.bincount(got['status'].ravel(), minlength=5)}, differ for {np.count_nonzero(differ)} of {B * N}")
    assert np.all(dx <= X_BAR)
    assert np.all(np.isin(got["status"], [0, 1, 2, 3]))
    if differ.any():                                         # only a pair the restatement itself is undecided about may differ
        _, unstable, _ = br.unstable_pairs(cs)
        assert np.count_nonzero(unstable) <= 0.02 * unstable.size and not np.any(differ & ~unstable)
    # summaries: against the restatement's replicates ...
    ref = br.summaries(want["x"], want["status"], RANKS)
    assert np.array_equal(got["n_used"], ref["n_used"]) and np.all(ref["n_used"] == B)
    bar = X_BAR * (1 + np.max(np.abs(want["x"]), axis=0))
    print(f"   order {np.max(np.abs(got['order'] - ref['order']) / bar):.2e}, mean {np.max(np.abs(got['mean'] - ref['mean']) / bar):.2e}, "
          f"sd {np.max(np.abs(got['sd'] - ref['sd']) / bar):.2e} (in units of the bar)")
    assert np.all(np.abs(got["order"] - ref["order"]) <= bar) and np.all(np.abs(got["mean"] - ref["mean"]) <= bar)
    assert np.all(np.abs(got["sd"] - ref["sd"]) <= np.sqrt(B / (B - 1.0)) * bar)
    # ... and against the rule applied to the device's own
    own = br.summaries(got["replicates"], got["status"], RANKS)
    assert np.array_equal(got["order"], own["order"]) and np.array_equal(got["n_used"], own["n_used"])
    assert np.allclose(got["mean"], own["mean"], rtol=1e-13, atol=0) and np.allclose(got["sd"], own["sd"], rtol=1e-13, atol=0)


# ----------------------------------------------------------------------------- 2. chunking and the subject split
def test_every_chunking_and_the_subject_split_give_the_same_bits():
    """N = 70: two workgroups, the second with six lanes.  B = 5 in launches of 1, 2 (2 + 2 + 1) and 5 replicates, and with
    the subjects split into passes of one workgroup."""
    c, center, sigma, noise = _cpep_inputs(70, 5)
    out = []
    for options in ((), (("bootstrap_chunk", 1),), (("bootstrap_chunk", 2),), (("bootstrap_chunk", 5),),
                    (("bootstrap_subjects", 64),), (("bootstrap_subjects", 64), ("bootstrap_chunk", 2))):
        _, eng, _ = _make("cpep-2441", 70, options=options)
        out.append(eng.bootstrap_conditional(sigma, 5, center, ranks=[0, 2, 4], noise=noise, upper=3.0, want_replicates=True))
        assert eng.n_failed() == 0
        eng.close()
    # (the synthetic population has a few flat subjects, who stay at their centre)
    assert np.all(out[0]["n_used"] == 5) and np.count_nonzero(np.std(out[0]["replicates"], axis=0) > 0) >= 60
    for o in out[1:]:
        _same(out[0], o)
    # the population's last subjects are their own, not the padding lanes' (lane 6 ... of the second workgroup)
    assert np.unique(out[0]["replicates"][:, 64:], axis=1).shape[1] == 6


# ----------------------------------------------------------------------------- 3. device draws
def test_device_draws_are_the_returned_noise_and_depend_on_nothing_else():
    from cude.engine import Engine
    from test_bootstrap_host import bootstrap_draw
    seed = 0x1234567890ABCDEF
    c, center, sigma, _ = _cpep_inputs(70, 5)
    _, eng, _ = _make("cpep-2441", 70)
    eng.set_rng(seed)
    kw = dict(ranks=[0, 4], upper=3.0, want_replicates=True)
    a = eng.bootstrap_conditional(sigma, 5, center, **kw)
    z = eng.bootstrap_noise(0, 5)
    T = len(c["tp"])
    assert z.shape == (5, T, 70) and np.all(z[:, 0, :] == 0.0) and not np.any(np.signbit(z[:, 0, :]))
    # the counter layout of csrc/cude_rng.h (Box-Muller through libm here: a few ulp)
    for b, r, i in ((0, 1, 0), (4, T - 1, 69), (2, 3, 33)):
        zn = bootstrap_draw(seed, i, b, r)
        assert abs(z[b, r, i] - zn) <= 4e-15 * max(1.0, abs(zn)), (b, r, i)
    assert 0.8 < z[:, 1:, :].std() < 1.2
    _same(a, eng.bootstrap_conditional(sigma, 5, center, noise=z, **kw))
    # a window of the replicates: the caller's first_rep, no hidden stream position
    w = eng.bootstrap_conditional(sigma, 2, center, first_rep=3, ranks=[0, 1], upper=3.0, want_replicates=True)
    assert np.array_equal(w["replicates"], a["replicates"][3:5]) and np.array_equal(w["status"], a["status"][3:5])
    assert np.array_equal(eng.bootstrap_noise(3, 2), z[3:5])
    # chunked generation draws the same numbers
    eng.set_option("bootstrap_chunk", 2)
    _same(a, eng.bootstrap_conditional(sigma, 5, center, **kw))
    assert np.array_equal(eng.bootstrap_noise(0, 5), z)
    eng.close()
    # a shard: subjects 30 ... 69 in a context of their own
    sl = slice(30, 70)
    e2 = Engine("cpep", (2, 4, 2), n_steps=30, n_state=2)
    e2.set_population_cpep(c["tp"], c["G"][sl], c["obs"][sl], c["age"][sl], c["t2dm"][sl])
    e2.set_params(c["nn"], None)
    e2.set_rng(seed, 30)
    s = e2.bootstrap_conditional(sigma[sl], 5, center[sl], **kw)
    assert np.array_equal(e2.bootstrap_noise(0, 5), z[:, :, sl])
    e2.close()
    for k in ("replicates", "status"):
        assert np.array_equal(s[k], a[k][:, sl]), k
    for k in ("mean", "sd", "n_used"):
        assert np.array_equal(s[k], a[k][sl]), k
    assert np.array_equal(s["order"], a["order"][:, sl])


# ----------------------------------------------------------------------------- 4. no noise
@pytest.mark.parametrize("name", ["cpep-2441", "supp-4355"])
def test_sigma_zero_returns_the_centre(name):
    import bootstrap_ref as br
    host = br.case(name, B=1)
    c, eng, spec = _make(name)
    box = spec[4]
    r = eng.bootstrap_conditional(0.0, 4, host["center"], ranks=[0, 3], lower=box[0], upper=box[1], want_replicates=True)
    eng.close()
    bar = X_BAR * (1 + np.abs(host["center"]))
    print(f"{name}: max |x - centre| {np.max(np.abs(r['replicates'] - host['center'])):.2e}, max sd {np.max(r['sd']):.2e}")
    assert np.all(r["status"] != 4) and np.all(r["n_used"] == 4)
    assert np.all(np.abs(r["replicates"] - host["center"]) <= bar) and np.all(r["sd"] <= bar)
    assert np.all(np.abs(r["mean"] - host["center"]) <= bar)


# ----------------------------------------------------------------------------- 5. stepped form = fused form
@pytest.mark.parametrize("name", ["cpep-2441", "supp-4355"])
def test_stepped_form_equals_fused_form(name):
    import bootstrap_ref as br
    host = br.case(name, B=3)
    out = []
    for fused in (1, 0):
        c, eng, spec = _make(name, options=(("refine_fused", fused),))
        box = spec[4]
        out.append(eng.bootstrap_conditional(host["sigma"], 3, host["center"], ranks=[0, 2], noise=host["noise"], lower=box[0],
                                             upper=box[1], want_replicates=True))
        eng.close()
    a, b = out
    dx = np.abs(a["replicates"] - b["replicates"]) / (1 + np.abs(a["replicates"]))
    print(f"{name}: max |dx|/(1+|x|) {dx.max():.2e}, statuses differ for {np.count_nonzero(a['status'] != b['status'])}")
    assert np.all(dx <= X_BAR) and np.array_equal(a["status"], b["status"]) and np.array_equal(a["n_used"], b["n_used"])


# ----------------------------------------------------------------------------- 6. adaptive mode
def test_adaptive_mode_never_ends_above_the_centre():
    """B = 3, N = 12.  Every replicate's data are rebuilt from public outputs (forward's trajectory at the centre, the noise
    passed in) and put into a context of their own: cude_forward's objective there is no higher at the replicate's estimate
    than at the centre, the start of its fit."""
    import bootstrap_ref as br
    from cude.engine import Engine
    from cude._lib import CudeError
    c, center, sigma, noise = _cpep_inputs(12, 3)
    _, eng, _ = _make("cpep-2441", 12, n_steps=0)
    yhat = _yhat(eng, center, False)
    r = eng.bootstrap_conditional(sigma, 3, center, ranks=[0, 2], noise=noise, upper=3.0, max_evals=20, want_replicates=True)
    with pytest.raises(CudeError):
        eng.adaptive_steps(0)                                # the last solve was of a trial point
    eng.close()
    assert np.all(np.isin(r["status"], [0, 1, 2, 3])) and np.all(r["n_used"] == 3)
    ystar = br.replicate_data(yhat, sigma, np.ones(1), noise, c["obs"].T[None])
    for b in range(3):
        e = Engine("cpep", (2, 4, 2), n_steps=0, n_state=2)
        e.set_population_cpep(c["tp"], c["G"], np.ascontiguousarray(ystar[b, 0].T), c["age"], c["t2dm"])
        e.set_params(c["nn"], center)
        f0 = e.forward(want_sse=True)["sse"]
        e.set_params(None, r["replicates"][b])
        f1 = e.forward(want_sse=True)["sse"]
        e.close()
        print(f"replicate {b}: max (F - F_centre) / F_centre {np.max((f1 - f0) / f0):.2e}; moved {np.count_nonzero(r['replicates'][b] != center)}")
        assert np.all(f1 <= f0 * (1 + 1e-12))
    assert np.count_nonzero(r["replicates"] != center[None]) >= 18


# ----------------------------------------------------------------------------- 7. failure isolation
def test_a_nan_centre_fails_its_subject_alone():
    c, center, sigma, noise = _cpep_inputs(70, 4)
    _, eng, _ = _make("cpep-2441", 70)
    kw = dict(ranks=[0, 3], noise=noise, upper=3.0, want_replicates=True)
    clean = eng.bootstrap_conditional(sigma, 4, center, **kw)
    bad = center.copy()
    bad[5] = np.nan
    r = eng.bootstrap_conditional(sigma, 4, bad, **kw)
    assert eng.n_failed() == 1
    eng.close()
    assert np.all(r["status"][:, 5] == 4) and r["n_used"][5] == 0
    assert np.isnan(r["mean"][5]) and np.isnan(r["sd"][5]) and np.all(np.isnan(r["order"][:, 5]))
    ok = np.arange(70) != 5
    for k in ("replicates", "status", "order"):
        assert np.array_equal(r[k][:, ok], clean[k][:, ok]), k
    for k in ("mean", "sd", "n_used"):
        assert np.array_equal(r[k][ok], clean[k][ok]), k


# ----------------------------------------------------------------------------- 8. arguments
def test_argument_errors_and_refusals():
    from cude.engine import Engine
    from cude._lib import CudeError
    c, center, sigma, noise = _cpep_inputs(24, 3)
    _, eng, _ = _make("cpep-2441", 24)
    cond = np.linspace(-1.0, 0.0, 24)
    eng.set_params(None, cond)
    a = eng.bootstrap_conditional(sigma, 3, None, noise=noise, upper=3.0, want_replicates=True)    # centre = NULL: the context's
    assert np.array_equal(eng.get_params()[1], cond)         # ... which stay what they were
    _same(a, eng.bootstrap_conditional(sigma, 3, cond, noise=noise, upper=3.0, want_replicates=True))

    def err(status=-1, **kw):
        args = dict(sigma=sigma, n_reps=3, center=cond, noise=noise, upper=3.0)
        args.update(kw)
        with pytest.raises(CudeError) as e:
            eng.bootstrap_conditional(args.pop("sigma"), args.pop("n_reps"), args.pop("center"), **args)
        assert e.value.status == status, (kw, e.value)
    neg, nan = sigma.copy(), sigma.copy()
    neg[3], nan[7] = -1e-3, np.nan
    err(sigma=neg)
    err(sigma=nan)
    err(sigma=np.full(24, np.inf))
    err(lower=1.0, upper=1.0)
    err(lower=-np.inf)
    err(max_evals=0)
    err(xtol=0.0)
    err(max_step=0.0)
    err(penalty_weight=-1.0)
    err(penalty_center=np.nan)
    err(n_reps=0, noise=None)
    err(n_reps=4097, noise=None)
    err(first_rep=-1, noise=None)
    err(ranks=[1, 1])
    err(ranks=[2, 1])
    err(ranks=[3])                                           # outside [0, n_reps)
    err(ranks=[-1])
    err(n_reps=20, noise=None, ranks=list(range(17)))        # more than 16 ranks
    lib, out = eng._lib, np.zeros(24)
    import ctypes as C
    p = lambda v: v.ctypes.data_as(C.c_void_p)               # noqa: E731
    base = [eng._h, None, p(sigma), 0, 3, None, -4.0, 3.0, 40, 1e-7, 0.5, 0.0, 0.0, 0, None, None, p(out), None, None, None, None]
    assert lib.cude_bootstrap_conditional(*base) == 0
    no_out = list(base)
    no_out[16] = None
    assert lib.cude_bootstrap_conditional(*no_out) == -1     # no output requested
    no_sigma = list(base)
    no_sigma[2] = None
    assert lib.cude_bootstrap_conditional(*no_sigma) == -1
    order_without_ranks = list(base)
    order_without_ranks[15] = p(out)
    assert lib.cude_bootstrap_conditional(*order_without_ranks) == -1
    assert lib.cude_bootstrap_noise(eng._h, 0, 0, p(out)) == -1 and lib.cude_bootstrap_noise(eng._h, 0, 1, None) == -1
    assert lib.cude_bootstrap_noise(eng._h, -1, 1, p(out)) == -1 and lib.cude_bootstrap_noise(eng._h, 0, 4097, p(out)) == -1
    eng.close()
    # CUDE_ERR_STATE: no shared parameters, no centre
    e1 = Engine("cpep", (2, 4, 2), n_steps=30, n_state=2)
    with pytest.raises(CudeError) as e:
        e1.bootstrap_noise(0, 1)                             # population not set
    assert e.value.status == -3
    e1.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
    with pytest.raises(CudeError) as e:
        e1.bootstrap_conditional(sigma, 3, cond)
    assert e.value.status == -3
    e1.set_params(c["nn"], None)
    with pytest.raises(CudeError) as e:
        e1.bootstrap_conditional(sigma, 3, None)
    assert e.value.status == -3
    e1.close()
    # the fallback kernel has no tangent solve
    eng = Engine("cpep", (2, [5, 3]), n_steps=30, n_state=2)
    assert eng.fallback_kernel
    eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
    eng.set_params(np.full(eng.P, 0.1), None)
    with pytest.raises(CudeError) as e:
        eng.bootstrap_conditional(sigma, 3, cond)
    assert e.value.status == -4 and "fallback" in str(e.value) and "no tangent-linear solve" in str(e.value)
    eng.close()


# ----------------------------------------------------------------------------- 9. the mirrors
def test_api_bootstrap_conditional_end_to_end(fixed_step_default):
    from conftest import make_cpep_case
    from cude import api
    N, B = 24, 40
    c = make_cpep_case(N, (2, 4, 2))
    net = api.chain(4, 2, input_dims=2)
    models = [api.CPeptideConditionalUDEModel(c["G"][i], c["tp"], c["age"][i], net, c["obs"][i], bool(c["t2dm"][i]))
              for i in range(N)]
    betas, sse = api.estimate_conditional(models, c["tp"], c["obs"], c["nn"], lower=-4.0, upper=3.0, n_steps=30, method="newton")
    noise = np.random.default_rng(9).standard_normal((B, len(c["tp"]), N))
    r = api.bootstrap_conditional(betas, c["nn"], models, c["tp"], c["obs"], n_reps=B, noise=noise, upper=3.0, n_steps=30,
                                  return_replicates=True)
    assert np.allclose(r.sigma, np.sqrt(sse / len(c["tp"])), rtol=1e-12)
    ok = r.n_used == B
    assert np.count_nonzero(ok) == N
    want = np.quantile(r.replicates, [0.025, 0.975], axis=0)
    assert np.allclose(r.lower, want[0], rtol=1e-14, atol=1e-14) and np.allclose(r.upper, want[1], rtol=1e-14, atol=1e-14)
    assert np.allclose(r.se, np.std(r.replicates, axis=0, ddof=1), rtol=1e-12)
    assert np.allclose(r.bias, r.replicates.mean(axis=0) - betas, rtol=0, atol=1e-13)
    assert np.all(r.lower <= r.upper) and np.all(r.se > 0)
    # the same call without the replicates; and the device stream, seeded: reproducible, another seed differs
    r2 = api.bootstrap_conditional(betas, c["nn"], models, c["tp"], c["obs"], n_reps=B, noise=noise, upper=3.0, n_steps=30)
    assert np.array_equal(r2.lower, r.lower) and np.array_equal(r2.se, r.se) and not hasattr(r2, "replicates")
    d1 = api.bootstrap_conditional(betas, c["nn"], models, c["tp"], c["obs"], n_reps=B, seed=5, upper=3.0, n_steps=30)
    d2 = api.bootstrap_conditional(betas, c["nn"], models, c["tp"], c["obs"], n_reps=B, seed=5, upper=3.0, n_steps=30)
    d3 = api.bootstrap_conditional(betas, c["nn"], models, c["tp"], c["obs"], n_reps=B, seed=6, upper=3.0, n_steps=30)
    assert np.array_equal(d1.se, d2.se) and not np.array_equal(d1.se, d3.se)
    api.clear_cache()


def test_api_suppression_bootstrap_end_to_end(fixed_step_default):
    from conftest import make_supp_case
    from cude import api
    N, B = 16, 24
    c = make_supp_case(N)
    prob = api.SuppressionProblem(api.chain(3, 5, input_dims=4))
    theta, _ = api.validate_suppression_model(None, prob, c["data"], c["tp"], c["nn"], n_steps=30, lower=-6.0, upper=4.0,
                                              method="newton")
    p = api.ComponentArray(theta=theta, neural=c["nn"])
    noise = np.random.default_rng(4).standard_normal((B, 3 * len(c["tp"]), N))
    r = api.suppression_bootstrap(p, (prob, c["data"], c["tp"], 0.0), sigma=0.05, n_reps=B, noise=noise, lower=-6.0, upper=4.0,
                                  n_steps=30, return_replicates=True)
    assert np.all(r.n_used == B)
    want = np.quantile(r.replicates, [0.025, 0.975], axis=0)
    assert np.allclose(r.lower, want[0], rtol=1e-14, atol=1e-14) and np.allclose(r.upper, want[1], rtol=1e-14, atol=1e-14)
    assert np.allclose(r.se, np.std(r.replicates, axis=0, ddof=1), rtol=1e-12) and np.all(r.se > 0)
    # sigma = None: the weighted SSE over the 3 T residual rows
    pop = api._supp_population(prob, c["data"], c["tp"], 0.0, 30)
    pop.engine.set_params(c["nn"], theta)
    sse = pop.engine.forward(want_sse=True)["sse"]
    r0 = api.suppression_bootstrap(p, (prob, c["data"], c["tp"], 0.0), n_reps=4, noise=noise[:4], lower=-6.0, upper=4.0, n_steps=30)
    assert np.allclose(r0.sigma, np.sqrt(sse / (3 * len(c["tp"]))), rtol=1e-12)
    api.clear_cache()
