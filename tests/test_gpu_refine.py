"""cude_refine_conditional on the device (csrc/cude_refine.hip): the one-launch Newton-type fits of every subject's
conditional parameter, against

  * the rule restated in numpy over the CPU oracle's tangent solves (tests/refine_ref.py, held against scipy's Brent on the
    C oracle by tests/test_refine_host.py);
  * the defining property of the result, through cude_forward alone;
  * the global search cude_fit_conditional on the subjects whose profile has one basin;
  * itself: stepped form = fused form, the adaptive mode's guarantees.

Bars.  tests/test_refine_host.py records, for the restatement under the error the tangent kernels are allowed (score and
info times 1 +- 1e-9), (a) = max |dx| / (1 + |x|) = 1.8e-14 and (b) = 0 of 24 / 0 of 16 subjects whose `evals` change, at
the default xtol = 1e-7.  Hence here: |x - x_ref| <= 10 max((a), xtol) (1 + |x|) = 1e-6 (1 + |x|), statuses equal, and
`evals` equal except for at most 2 (b) of the subjects -- that is: equal.  Every case below was put through the same
perturbation on the CPU before it was admitted (no status and no `evals` changed)."""
import numpy as np
import pytest
import torch  # noqa: F401

from conftest import make_cpep_case, make_supp_case

pytestmark = pytest.mark.gpu

XTOL = 1e-7
A_RECORDED = 1.8e-14
X_BAR = 10.0 * max(A_RECORDED, XTOL)
B_SHARE = 0.0                       # (b): largest share of subjects whose evals change under the perturbation
PEN = (0.35, -0.6)


def _evals_bar(N):
    return int(2 * B_SHARE * N)


# ----------------------------------------------------------------------------- cases
# name -> (model, arch, n_state, N, box, constant start, max_step, cond_space, seed of the population)
CASES = {
    "cpep-2441": ("cpep", (2, 4, 2), 2, 24, (-4.0, 3.0), 0.0, 0.5, "log", 20250905),
    "cpep-2661": ("cpep", (2, 6, 2), 2, 24, (-4.0, 3.0), 0.0, 0.5, "log", 20250905),
    "cpep-2661-ns3": ("cpep", (2, 6, 2), 3, 24, (-4.0, 3.0), 0.0, 0.5, "log", 20250905),
    # (the default seed's covariate population has subjects that crawl along a plateau to max_evals, where the count of
    # evaluations is decided by rounding: not admissible under the perturbation rule of the module docstring)
    "cpep-3441": ("cpep", (3, 4, 2), 2, 24, (-4.0, 3.0), 0.0, 0.5, "log", 11),
    "sym-raw": ("cpep_sym", (1, 0, 0), 2, 24, (0.5, 400.0), 20.0, 10.0, "raw", 20250905),
    "supp-4355": ("supp", (4, 3, 5), 3, 16, (-6.0, 4.0), 0.0, 0.5, "log", 7),
}
SYM_P0, SYM_STEPS = 1.78, 32


def _case_data(name, N=None):
    """The population of a case: conftest's, and for the symbolic model observations of its own (conftest's come from a
    network the Michaelis-Menten production cannot follow: every k would run to the upper bound) -- the oracle's forward
    solve of the symbolic model at k = 20 exp(beta) with 5 % multiplicative noise."""
    model, arch, n_state, n_def, box, x_const, max_step, space, seed = CASES[name]
    N = n_def if N is None else N
    if model == "supp":
        return make_supp_case(N, arch, seed=seed)
    c = make_cpep_case(N, arch if model == "cpep" else (2, 4, 2), seed=seed)
    if model == "cpep_sym":
        import cude_oracle as o
        pop = o.CPepPopulation(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"], covariate=False)
        k_true = 20.0 * np.exp(c["beta"])
        traj = o.cpep_forward(np, np.array([SYM_P0]), k_true, pop, (1, 0, 0), SYM_STEPS, 2, "raw")
        u1 = np.stack([np.broadcast_to(np.asarray(traj[t][0], dtype=np.float64), (N,)) for t in range(len(c["tp"]))], axis=1)
        obs = u1 * (1.0 + 0.05 * np.random.default_rng(seed + 2).standard_normal(u1.shape))
        obs[:, 0] = c["obs"][:, 0]
        c = dict(c, obs=obs, nn=np.array([SYM_P0]))
    return dict(c, arch=arch)


def _evaluator(name, c):
    import refine_ref as rr
    model, arch, n_state, _, _, _, _, space, _ = CASES[name]
    if model == "supp":
        return lambda **kw: rr.supp_evaluator(c, **kw)
    steps = 30 if model == "cpep" else SYM_STEPS
    return lambda **kw: rr.cpep_evaluator(c, n_steps=steps, n_state=n_state, cond_space=space, **kw)


def _make(name, N=None, n_steps=30):
    """(case data, engine with the shared parameters set, restatement's evaluation factory)."""
    from cude.engine import Engine
    model, arch, n_state, n_def, box, x_const, max_step, space, _ = CASES[name]
    c = _case_data(name, N)
    N = n_def if N is None else N
    if model == "supp":
        eng = Engine("supp", arch, n_steps=n_steps)
        eng.set_population_supp(c["tp"], c["data"])
    else:
        eng = Engine(model, arch, n_steps=n_steps if model == "cpep" or n_steps == 0 else SYM_STEPS, n_state=n_state,
                     cond_space=space)
        eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
    eng.set_params(c["nn"], np.full(N, x_const))
    return c, eng, _evaluator(name, c)


def _starts(name, ev, N, pw, pc):
    import refine_ref as rr
    box, x_const = CASES[name][4], CASES[name][5]
    values, prof = rr.scan(ev, N, *box)
    pen = prof + pw * (values[:, None] - pc) ** 2
    return {"scan": values[np.argmin(pen, axis=0)], "const": np.full(N, x_const)}, values, prof


def _F(eng, x, pw=0.0, pc=0.0):
    eng.set_params(None, x)
    return eng.forward(want_sse=True)["sse"] + pw * (x - pc) ** 2


# ----------------------------------------------------------------------------- 1. fused form vs the restatement
@pytest.mark.parametrize("penalty", [False, True], ids=["plain", "penalised"])
@pytest.mark.parametrize("name", list(CASES))
def test_fused_form_follows_the_restatement(name, penalty):
    import refine_ref as rr
    c, eng, make_ev = _make(name)
    N, box, max_step = CASES[name][3], CASES[name][4], CASES[name][6]
    pw, pc = PEN if penalty else (0.0, 0.0)
    if name == "sym-raw" and penalty:
        pw, pc = 1e-4, 20.0                                  # (k itself: a penalty on the scale of k)
    ev = make_ev()
    starts, _, _ = _starts(name, ev, N, pw, pc)
    for tag, x0 in starts.items():
        want = rr.refine(ev, x0, *box, xtol=XTOL, max_step=max_step, pw=pw, pc=pc)
        got = eng.refine_conditional(x0, box[0], box[1], xtol=XTOL, max_step=max_step, penalty_weight=pw, penalty_center=pc)
        dx = np.abs(got["x"] - want["x"]) / (1 + np.abs(want["x"]))
        de = np.abs(got["evals"].astype(int) - want["evals"])
        print(f"{name} {tag} pw={pw}: max |dx|/(1+|x|) {dx.max():.2e}; evals ref {want['evals'].min()}..{want['evals'].max()}, "
              f"differ for {np.count_nonzero(de)} of {N} (max {de.max()}); status ref {np.bincount(want['status'], minlength=5)} "
              f"dev {np.bincount(got['status'], minlength=5)}")
        assert np.all(dx <= X_BAR)
        assert np.array_equal(got["status"], want["status"])
        assert np.count_nonzero(de) <= _evals_bar(N) and de.max() <= 1
        # the outputs belong to the returned point
        sse = _F(eng, got["x"])
        sens = eng.sensitivity(want_sens=False)
        info = sens["info"]
        print(f"   sse vs cude_forward: max rel {np.max(np.abs(got['sse'] - sse) / sse):.2e} (smallest SSE {sse.min():.2e}); "
              f"vs cude_sensitivity's: {np.max(np.abs(got['sse'] - sens['sse']) / sse):.2e}; "
              f"info vs cude_sensitivity: {np.max(np.abs(got['info'] - info)) / np.max(info):.2e}")
        assert np.all(np.abs(got["sse"] - sse) <= 1e-12 * sse)
        assert np.allclose(got["objective"], got["sse"] + pw * (got["x"] - pc) ** 2, rtol=1e-12, atol=0.0)
        assert np.max(np.abs(got["info"] - info)) <= 1e-9 * np.max(info)
        assert eng.n_failed() == 0
    eng.close()


# ----------------------------------------------------------------------------- 2. the defining property
@pytest.mark.parametrize("name", ["cpep-2661", "cpep-3441", "supp-4355"])
def test_result_is_a_local_minimiser_and_never_worse_than_the_start(name):
    c, eng, _ = _make(name, N=150)
    box = CASES[name][4]
    for pw, pc in ((0.0, 0.0), PEN):
        x0 = np.linspace(box[0] - 0.5, box[1] + 0.5, 150)           # starts all over the box, some outside it
        r = eng.refine_conditional(x0, *box, penalty_weight=pw, penalty_center=pc)
        x = r["x"]
        F = _F(eng, x, pw, pc)                                      # (every value below is cude_forward's)
        assert np.all((x >= box[0]) & (x <= box[1])) and np.all(np.isin(r["status"], [0, 1, 2, 3]))
        F_start = _F(eng, np.clip(x0, *box), pw, pc)
        print(f"{name} pw={pw}: max (F - F_start) {np.max(F - F_start):.3e}, max |F - objective_out| / F {np.max(np.abs(F - r['objective']) / F):.2e}")
        assert np.all(F <= F_start)
        conv = r["status"] == 0
        print(f"{name} pw={pw}: status {np.bincount(r['status'], minlength=5)}, evals {r['evals'].min()}..{r['evals'].max()}")
        assert np.count_nonzero(conv) >= 75
        for d in (1e-4, -1e-4):
            inside = conv & (x + d > box[0]) & (x + d < box[1])
            assert np.all(_F(eng, x + d, pw, pc)[inside] >= F[inside] - 1e-10)
    eng.close()


# ----------------------------------------------------------------------------- 3. against the global search
@pytest.mark.parametrize("name", ["cpep-2441", "supp-4355"])
def test_same_minimiser_as_the_search_on_unique_basins(name):
    import refine_ref as rr
    c, eng, _ = _make(name)
    N, box = CASES[name][3], CASES[name][4]
    values = np.linspace(box[0], box[1], 41)
    prof = eng.profile_conditional(values)
    xs, fs, _ = eng.fit_conditional(box[0], box[1], 41, 48)
    r = eng.refine_conditional(values[np.argmin(prof, axis=0)], *box)
    checked = 0
    for i in range(N):
        if rr.unique_interior_basin(prof, i) is None:
            continue
        print(f"subject {i}: |dx| {abs(r['x'][i] - xs[i]):.2e}, (F - F_search) / F {(r['objective'][i] - fs[i]) / fs[i]:.2e}")
        assert abs(r["x"][i] - xs[i]) < 2e-6 and r["objective"][i] <= fs[i] * (1 + 1e-10)
        checked += 1
    assert checked >= N // 2
    eng.close()


# ----------------------------------------------------------------------------- 4. stepped form = fused form
@pytest.mark.parametrize("name", ["cpep-2661-ns3", "sym-raw", "supp-4355"])
def test_stepped_form_equals_fused_form(name):
    """The stepped form runs the sensitivity kernels, the fused form the fit kernels: a fork of the sweep they share, or of
    the rule, shows here as a differing bit."""
    out = []
    N, box, x_const, max_step = CASES[name][3], CASES[name][4], CASES[name][5], CASES[name][6]
    for fused in (1, 0):
        c, eng, _ = _make(name, N=65)
        eng.set_option("refine_fused", fused)
        out.append(eng.refine_conditional(np.full(65, x_const), *box, max_step=max_step, penalty_weight=PEN[0] * (name != "sym-raw"),
                                          penalty_center=PEN[1]))
        eng.close()
    a, b = out
    dx = np.abs(a["x"] - b["x"]) / (1 + np.abs(a["x"]))
    print(f"{name}: max |dx|/(1+|x|) {dx.max():.2e}, evals differ for {np.count_nonzero(a['evals'] != b['evals'])}")
    # bit for bit: both forms evaluate through the one sweep of csrc/cude_tangent.h and judge by the one refine_update
    assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["evals"], b["evals"]) and np.array_equal(a["status"], b["status"])


# ----------------------------------------------------------------------------- 5. adaptive mode
def _oracle_sse(name, c, x, mode):
    """Per-subject SSE on the CPU oracle: mode "adaptive" or the fixed-step solve with 480 steps."""
    import c_oracle as co
    import cude_oracle as o
    if name.startswith("supp"):
        if mode == "adaptive":
            u = co.supp_adaptive(c["tp"], c["data"], c["arch"], c["nn"], x)
            return (((u - c["data"]) / o.supp_scale(c["data"])[:, None, None]) ** 2).sum(axis=(0, 1))
        return co.supp(c["tp"], c["data"], c["arch"], c["nn"], x, 0.0, 480, want_grad=False)["sse"]
    if mode == "adaptive":
        u = co.cpep_adaptive(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"], c["arch"], c["nn"], np.exp(x), c["tp"])
        return ((u - c["obs"]) ** 2).sum(axis=1)
    return co.cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"], c["arch"], c["nn"], x, 480, 2, want_grad=False)["sse"]


@pytest.mark.parametrize("name", ["cpep-2441", "supp-4355"])
def test_adaptive_mode(name):
    """The stepped form over the adaptive tangent solve.  Step control makes the objective piecewise smooth: it jumps where
    the accepted-step sequence changes, so a local method may stop at a jump and is compared with the search only up to
    the jumps' size.  eps = max over the subjects and a 201-point grid of +-0.05 around the search's minimiser of
    |SSE_adaptive - SSE_fixed(S = 480)| on the CPU oracle, printed below (3.1e-4 for the c-peptide case, 0.17 for the
    suppression case when this was written, where max (F_refine - F_search) was 2.0e-4 resp. 0.15);
    F_refine <= F_search + 4 eps."""
    from cude._lib import CudeError
    c, eng, _ = _make(name, N=None, n_steps=0)
    N, box = CASES[name][3], CASES[name][4]
    x0 = np.zeros(N)
    F0 = _F(eng, x0)
    r40 = eng.refine_conditional(x0, *box, max_evals=40)
    with pytest.raises(CudeError):
        eng.adaptive_steps(0)                                # the last solve was of a trial point
    r20 = eng.refine_conditional(x0, *box, max_evals=20)
    print(f"{name}: status {np.bincount(r40['status'], minlength=5)}, evals {r40['evals'].min()}..{r40['evals'].max()}")
    assert np.all(np.isin(r40["status"], [0, 1, 2, 3])) and eng.n_failed() == 0
    assert np.all(r40["objective"] <= F0 * (1 + 1e-12))
    done = r20["status"] != 2
    print(f"{name}: {np.count_nonzero(done)} of {N} subjects finish within 20 evaluations")
    assert np.count_nonzero(done) >= 1
    for k in ("x", "objective", "sse", "info", "evals", "status"):
        assert np.array_equal(r20[k][done], r40[k][done]), k
    sse = _F(eng, r40["x"])
    assert np.all(np.abs(r40["sse"] - sse) <= 1e-12 * sse)
    xs, fs, _ = eng.fit_conditional(box[0], box[1], 41, 48)
    eps = 0.0
    for d in np.linspace(-0.05, 0.05, 201):
        eps = max(eps, float(np.max(np.abs(_oracle_sse(name, c, xs + d, "adaptive") - _oracle_sse(name, c, xs + d, "fixed")))))
    print(f"{name}: eps = {eps:.3e}; max (F_refine - F_search) = {np.max(r40['objective'] - fs):.3e}")
    assert np.all(r40["objective"] <= fs + 4 * eps)
    eng.close()


# ----------------------------------------------------------------------------- 6. context, sizes, order
def test_context_parameters_sizes_and_argument_errors():
    from cude.engine import Engine
    from cude._lib import CudeError
    name = "cpep-2441"
    box = CASES[name][4]
    c, eng, _ = _make(name, N=65)                            # a partial second wave
    cond = np.linspace(-1.5, 0.5, 65)
    eng.set_params(None, cond)
    a = eng.refine_conditional(None, *box)                   # x0 = NULL: the context's conditional parameters
    assert np.array_equal(eng.get_params()[1], cond)         # ... which stay what they were
    b = eng.refine_conditional(cond, *box)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for bad in (dict(lower=1.0, upper=1.0), dict(max_evals=0), dict(xtol=0.0), dict(max_step=0.0), dict(penalty_weight=-1.0)):
        kw = dict(lower=box[0], upper=box[1])
        kw.update(bad)
        with pytest.raises(CudeError):
            eng.refine_conditional(cond, **kw)
    # one subject = the same subject inside a population
    c1 = {k: (v[:1] if k in ("G", "obs", "age", "t2dm") else v) for k, v in c.items()}
    e1 = Engine("cpep", (2, 4, 2), n_steps=30, n_state=2)
    e1.set_population_cpep(c1["tp"], c1["G"], c1["obs"], c1["age"], c1["t2dm"])
    with pytest.raises(CudeError):
        e1.refine_conditional(np.zeros(1), *box)             # shared parameters not set
    e1.set_params(c["nn"], None)
    with pytest.raises(CudeError):
        e1.refine_conditional(None, *box)                    # no start
    r1 = e1.refine_conditional(cond[:1], *box)
    assert r1["x"][0] == a["x"][0] and r1["evals"][0] == a["evals"][0] and r1["status"][0] == a["status"][0]
    e1.close()
    eng.close()
    # a failed subject, a flat one, a box that excludes the basin, two evaluations
    G = c["G"].copy()
    G[9, 2] = np.nan
    G[5, :] = G[5, 0]
    eng = Engine("cpep", (2, 4, 2), n_steps=30, n_state=2)
    eng.set_population_cpep(c["tp"], G, c["obs"], c["age"], c["t2dm"])
    eng.set_params(c["nn"], None)
    r = eng.refine_conditional(np.full(65, 5.0), *box)
    assert r["status"][9] == 4 and r["x"][9] == 3.0 and np.isposinf(r["objective"][9]) and eng.n_failed() == 1
    assert r["status"][5] == 3 and r["evals"][5] == 1 and r["info"][5] == 0.0
    ok = np.ones(65, bool)
    ok[[5, 9]] = False
    r2 = eng.refine_conditional(cond, *box)
    assert np.array_equal(r2["x"][ok], a["x"][ok]) and np.array_equal(r2["evals"][ok], a["evals"][ok])
    lo, hi = a["x"][0] + 0.2, a["x"][0] + 0.7
    rb = eng.refine_conditional(np.full(65, hi), lo, hi)
    assert a["status"][0] == 0 and rb["status"][0] == 1 and rb["x"][0] == lo
    rm = eng.refine_conditional(np.zeros(65), *box, max_evals=2)
    flat = rm["status"] == 3                                 # (the synthetic population has flat subjects of its own)
    assert np.all(rm["status"][ok & ~flat] == 2) and np.all(rm["evals"][ok & ~flat] == 2) and np.count_nonzero(flat) <= 6
    eng.close()
    # the fallback kernel has no tangent solve
    eng = Engine("cpep", (2, [5, 3]), n_steps=30, n_state=2)
    assert eng.fallback_kernel
    eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
    eng.set_params(np.full(eng.P, 0.1), None)
    with pytest.raises(CudeError) as e:
        eng.refine_conditional(cond, *box)
    assert e.value.status == -4 and "fallback" in str(e.value)            # CUDE_ERR_UNSUPPORTED
    eng.close()


def test_large_population_smoke():
    name = "cpep-2661"
    box = CASES[name][4]
    c, eng, _ = _make(name, N=10000)
    r = eng.refine_conditional(np.zeros(10000), *box)
    print(f"1e4: status {np.bincount(r['status'], minlength=5)}, evals mean {r['evals'].mean():.2f} max {r['evals'].max()}")
    assert np.all(np.isin(r["status"], [0, 1, 2, 3])) and np.count_nonzero(r["status"] == 0) >= 7500
    assert np.all(_F(eng, r["x"]) <= _F(eng, np.zeros(10000)))
    eng.close()


def test_regrouped_population_keeps_the_subjects_indices():
    name = "cpep-2441"
    box = CASES[name][4]
    out = []
    for regroup in (False, True):
        c, eng, _ = _make(name, N=200, n_steps=0)
        x0 = np.linspace(-2.0, 0.5, 200)
        if regroup:
            eng.set_params(None, x0)
            eng.loss_grad()
            eng.adaptive_regroup()
        out.append(eng.refine_conditional(x0, *box, max_evals=12))
        eng.close()
    a, b = out
    assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["evals"], b["evals"])
    assert np.allclose(a["x"], b["x"], rtol=0.0, atol=1e-12) and np.allclose(a["sse"], b["sse"], rtol=1e-12, atol=0.0)


# ----------------------------------------------------------------------------- 7. the mirror
def test_api_newton_against_search(fixed_step_default):
    import refine_ref as rr
    from cude import api
    N = 24
    c = make_cpep_case(N, (2, 4, 2))
    net = api.chain(4, 2, input_dims=2)
    models = [api.CPeptideConditionalUDEModel(c["G"][i], c["tp"], c["age"][i], net, c["obs"][i], bool(c["t2dm"][i]))
              for i in range(N)]
    kw = dict(lower=-4.0, upper=3.0, n_steps=30)
    xs, ss = api.estimate_conditional(models, c["tp"], c["obs"], c["nn"], **kw)
    xn, sn, info = api.estimate_conditional(models, c["tp"], c["obs"], c["nn"], method="newton", return_info=True, **kw)
    pop = api._population(models, c["tp"], c["obs"], 30)
    prof = pop.engine.profile_conditional(np.linspace(-4.0, 3.0, 41))
    uniq = np.array([rr.unique_interior_basin(prof, i) is not None for i in range(N)])
    assert np.count_nonzero(uniq) >= N // 2
    print(f"estimate_conditional: max |dx| on unique basins {np.max(np.abs(xn - xs)[uniq]):.2e}")
    assert np.all(np.abs(xn - xs)[uniq] < 2e-6) and np.all(sn[uniq] <= ss[uniq] * (1 + 1e-10))
    # the fit's info is what the standard errors need
    se_fit = api.conditional_standard_errors(xn, c["nn"], models, c["tp"], c["obs"], n_steps=30, info=info, sse=sn)
    se = api.conditional_standard_errors(xn, c["nn"], models, c["tp"], c["obs"], n_steps=30)
    assert np.allclose(se_fit, se, rtol=1e-8)
    sols = api.train(models, c["tp"], c["obs"], c["nn"], lbfgs_lower_bound=-4.0, lbfgs_upper_bound=3.0, n_steps=30, method="newton")
    assert np.array_equal(np.array([s.u[0] for s in sols]), xn)
    # MAPs: the search from the box, the refinement from the search's result moved off by 0.05
    sigma, omega = 0.3, 1.2
    ms = api.compute_individual_maps(None, c["nn"], models, c["tp"], c["obs"], sigma, omega, prior_individual=-1.0, n_steps=30)
    mn = api.compute_individual_maps(ms + 0.05, c["nn"], models, c["tp"], c["obs"], sigma, omega, prior_individual=-1.0,
                                     n_steps=30, method="newton")
    pen = prof + (sigma / omega) ** 2 * (np.linspace(-4.0, 3.0, 41)[:, None] + 1.0) ** 2
    uniq = np.array([rr.unique_interior_basin(pen, i) is not None for i in range(N)])
    print(f"compute_individual_maps: max |dx| on unique basins {np.max(np.abs(mn - ms)[uniq]):.2e}")
    assert np.count_nonzero(uniq) >= N // 2 and np.all(np.abs(mn - ms)[uniq] < 2e-6)
    api.clear_cache()
