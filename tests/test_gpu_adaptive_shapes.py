"""Every compiled adaptive kernel, forward and gradient, for every shape it is compiled for -- on inputs that exercise
every weight (tests/adaptive_cases.py: live biases, a scaled age column; its docstring says which case reaches which
kernel; tests/test_adaptive_cases_host.py shows on the oracle alone that the inputs are adequate).

  a. c-peptide on five knots, all 24 shapes: the team of waves ("adaptive_team" = 1, the eight shapes it is compiled
     for) and the unrolled one-wave kernel ("adaptive_team" = 0, and every other shape);
  b. c-peptide on six knots, all 24 shapes: the one-body kernel of the three translation units;
  c. suppression, all 16 shapes: the unrolled kernel (four shapes) and the one-body kernel (twelve);
  d. lanes that fail beside lanes that go on, on the two one-body kernels;
  e. the fixed-step kernels of every shape on the same inputs (live biases).

Checker and tolerances are those of tests/test_gpu_adaptive_grad.py and tests/test_gpu_round5.py: the oracle replays the
DEVICE's accepted steps and differentiates them by the complex-step method -- loss and per-subject SSE to 1e-10 (SSE of
the largest), gradients to 1e-8 of the reference array's max-norm; team against one-wave kernel: forward results bit for
bit, gradients to 1e-13.  Per block of the network gradient (each layer's weights, each layer's biases) the same
comparison is printed and asserted at min(1e-8 x the whole gradient's max-norm, 1e-5 x the block's own): no more than the
global bound already says given the 1e-3 floor of the host test, but a failure names the block.  That the device's
sequence is the oracle's own adaptive one: per shape at least 12 of 16 (63 of 70) subjects with the same number of steps
and every dt within 1e-3 of the span, and 90 % over all shapes together (the bar of test_cpep_adaptive_gradient; the
per-shape floor is there because a controller error in one shape's instantiation would fail all of that shape's
subjects).

Every figure is printed before it is asserted (pytest -s shows them; DESIGN.md records the worst per family)."""
import functools
import math

import numpy as np
import pytest

import adaptive_cases as ac

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-10           # tests/test_gpu_parity.py, for the fixed-step sweep
GRAD_RTOL = 1e-9

GRIDS = {"TP5": ac.TP5, "TP6": ac.TP6}
CPEP_IDS = [str(a) for a in ac.CPEP_SHAPES]
SUPP_IDS = [str(s) for s in ac.SUPP_SHAPES]


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _sets(nn, cond, seed):
    rng = np.random.default_rng(seed)
    nn_sets = nn[None, :] * (1.0 + 0.05 * rng.standard_normal((3, nn.size)))
    return nn_sets, cond[None, :] + 0.1 * rng.standard_normal((3, cond.size))


def _rows_are_single_calls(eng, nn_sets, cond_sets):
    """cude_multistart_loss_grad: every row equals its own cude_loss_grad call bit for bit."""
    L, Gn, Gc = eng.multistart_loss_grad(nn_sets, cond_sets)
    assert np.all(np.isfinite(L))
    for q in range(len(L)):
        eng.set_params(nn_sets[q], cond_sets[q])
        l1, gn1, gc1 = eng.loss_grad()
        assert l1 == L[q] and np.array_equal(gn1, Gn[q]) and np.array_equal(gc1, Gc[q]), q


def _blocks(tag, g, ref, arch):
    """Per block (a layer's weights, a layer's biases): |g - ref| against min(1e-8 max|ref|, 1e-5 max|ref[block]|);
    returns the worst error / bound."""
    top, worst, bad = float(np.max(np.abs(ref))), 0.0, []
    for name, s in ac.layer_blocks(arch):
        own = float(np.max(np.abs(ref[s])))
        err, bound = float(np.max(np.abs(g[s] - ref[s]))), min(1e-8 * top, 1e-5 * own)
        print(f"{tag} block {name}: |ref| {own:.3e} ({own / top:.1e} of the largest)  error {err:.3e}  bound {bound:.3e}")
        worst = max(worst, err / bound)
        if not err <= bound:
            bad.append((name, err, bound))
    assert not bad, bad
    return worst


# ----------------------------------------------------------------------------- a, b: c-peptide
@functools.lru_cache(maxsize=None)
def _cpep(grid, k):
    """Device results of both engines and the oracle's for cpep_case(CPEP_SHAPES[k], k, grid): computed once, read by
    the shape's own test and by the count over all shapes."""
    import cude_oracle as o
    from cude.engine import Engine
    arch = ac.CPEP_SHAPES[k]
    N = ac.cpep_subjects(arch)
    c = ac.cpep_case(arch, k, GRIDS[grid], N)
    pop = ac.cpep_population(c)
    nn_sets, b_sets = _sets(c["nn"], c["beta"], 4 + k)
    runs = []
    for team in (1, 0):
        eng = Engine("cpep", arch, n_steps=0, n_state=2)
        eng.set_option("adaptive_team", team)
        eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
        eng.set_params(c["nn"], c["beta"])
        fwd = eng.forward(want_sse=True, want_traj=True)
        loss, g_nn, g_b = eng.loss_grad()
        failed = eng.n_failed()
        steps = [eng.adaptive_steps(i) for i in range(N)]
        _rows_are_single_calls(eng, nn_sets, b_sets)
        eng.close()
        runs.append(dict(fwd=fwd, loss=loss, g_nn=g_nn, g_b=g_b, steps=steps, failed=failed))
    steps = runs[0]["steps"]
    replay = o.cpep_replay_loss_grad(c["nn"], c["beta"], pop, arch, [list(zip(t, dt)) for t, dt in steps])
    span = c["tp"][-1] - c["tp"][0]
    same = sum(ac.same_steps(ac.cpep_solve(c, pop, i)[1], *steps[i], span, 1e-3) for i in range(N))
    own = o.cpep_adaptive_loss_grad(c["nn"], c["beta"], pop, arch)
    return dict(arch=arch, N=N, c=c, runs=runs, replay=replay, same=same, own=own)


def _check_cpep(grid, k):
    r = _cpep(grid, k)
    arch, N, c = r["arch"], r["N"], r["c"]
    tag = f"cpep {grid} {arch}"
    team, wave = r["runs"]
    for run in r["runs"]:
        assert run["failed"] == 0 and np.isfinite(run["loss"])
        # the forward half of the gradient launch is the forward launch
        assert abs(run["loss"] - run["fwd"]["loss"]) <= 1e-14 * run["loss"]
        for t, dt in run["steps"]:                                   # a partition of the time span
            assert 8 <= len(t) <= 200
            assert t[0] == c["tp"][0] and np.all(t[1:] == t[:-1] + dt[:-1]) and abs(t[-1] + dt[-1] - c["tp"][-1]) < 1e-12
    # the two engines: the team against the one-wave kernel where the team applies, the same kernel twice elsewhere
    assert team["fwd"]["loss"] == wave["fwd"]["loss"] and np.array_equal(team["fwd"]["sse"], wave["fwd"]["sse"])
    assert np.array_equal(team["fwd"]["traj"], wave["fwd"]["traj"])
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(team["steps"], wave["steps"]))
    assert abs(team["loss"] - wave["loss"]) <= 1e-14 * abs(wave["loss"])
    print(f"{tag} engines: g_nn {_rel(team['g_nn'], wave['g_nn']):.2e}  g_cond {_rel(team['g_b'], wave['g_b']):.2e}")
    assert _rel(team["g_nn"], wave["g_nn"]) <= 1e-13 and _rel(team["g_b"], wave["g_b"]) <= 1e-13
    # (1) the adjoint of the device's own sequence (one replay serves both engines: their steps are the same bits)
    rl, rg, rb, rsse = r["replay"]
    for name, run in (("team=1", team), ("team=0", wave)):
        fig = (abs(run["loss"] - rl) / rl, _rel(run["fwd"]["sse"], rsse), _rel(run["g_nn"], rg), _rel(run["g_b"], rb))
        print(f"{tag} {name} replay: loss {fig[0]:.2e}  sse {fig[1]:.2e}  g_nn {fig[2]:.2e}  g_cond {fig[3]:.2e}")
        assert fig[0] <= 1e-10 and fig[1] <= 1e-10 and fig[2] <= 1e-8 and fig[3] <= 1e-8
        worst = _blocks(f"{tag} {name}", run["g_nn"], rg, arch)
        print(f"{tag} {name} worst block: {worst:.2e} of its bound")
    # (2) that sequence is the oracle's adaptive one
    print(f"{tag} controller: {r['same']} of {N} subjects take the oracle's steps")
    assert r["same"] >= (63 if N == 70 else 12)
    # (3) end to end against the oracle's own adaptive gradient, at the solver's tolerance
    ol, og, ob, _ = r["own"]
    print(f"{tag} own steps: loss {abs(team['loss'] - ol) / ol:.2e}  g_nn {_rel(team['g_nn'], og):.2e}")
    for run in r["runs"]:
        assert abs(run["loss"] - ol) <= 1e-4 * ol and _rel(run["g_nn"], og) <= 5e-3


@pytest.mark.parametrize("k", range(len(ac.CPEP_SHAPES)), ids=CPEP_IDS)
def test_cpep_five_knots_team_and_unrolled(k):
    _check_cpep("TP5", k)


@pytest.mark.parametrize("k", range(len(ac.CPEP_SHAPES)), ids=CPEP_IDS)
def test_cpep_six_knots_one_body(k):
    _check_cpep("TP6", k)


# ----------------------------------------------------------------------------- c: suppression
@pytest.mark.parametrize("k", range(len(ac.SUPP_SHAPES)), ids=SUPP_IDS)
def test_supp_unrolled_and_one_body(k):
    import cude_oracle as o
    from cude.engine import Engine
    N, lam = 12, 0.01
    s = ac.supp_case(ac.SUPP_SHAPES[k], k, N)
    arch, tag = s["arch"], f"supp {ac.SUPP_SHAPES[k]}"
    eng = Engine("supp", arch, n_steps=0, lam=lam)
    eng.set_population_supp(s["tp"], s["data"])
    eng.set_params(s["nn"], s["theta"])
    fwd = eng.forward(want_sse=True)
    loss, g_nn, g_t = eng.loss_grad()
    assert eng.n_failed() == 0 and abs(loss - fwd["loss"]) <= 1e-14 * loss
    steps = [eng.adaptive_steps(i) for i in range(N)]
    _rows_are_single_calls(eng, *_sets(s["nn"], s["theta"], 40 + k))
    eng.close()
    for t, dt in steps:
        assert 8 <= len(t) <= 200
        assert t[0] == s["tp"][0] and np.all(t[1:] == t[:-1] + dt[:-1]) and abs(t[-1] + dt[-1] - s["tp"][-1]) < 1e-12
    # (1) the adjoint of the device's own sequences
    rl, rg, rt, rsse = o.supp_replay_loss_grad(s["nn"], s["theta"], s["data"], s["tp"], arch, lam,
                                               [list(zip(t, dt)) for t, dt in steps])
    fig = (abs(loss - rl) / rl, _rel(fwd["sse"], rsse), _rel(g_nn, rg), _rel(g_t, rt))
    print(f"{tag} replay: loss {fig[0]:.2e}  sse {fig[1]:.2e}  g_nn {fig[2]:.2e}  g_cond {fig[3]:.2e}")
    assert fig[0] <= 1e-10 and fig[1] <= 1e-10 and fig[2] <= 1e-8 and fig[3] <= 1e-8
    # (per block without the penalty's share 2 lambda nn, which is not the kernel's work)
    worst = _blocks(tag, g_nn - 2.0 * lam * s["nn"], rg - 2.0 * lam * s["nn"], arch)
    print(f"{tag} worst block: {worst:.2e} of its bound")
    # (2) the oracle's own adaptive solve and gradient
    ol, og, ot, _ = o.supp_adaptive_loss_grad(s["nn"], s["theta"], s["data"], s["tp"], arch, lam)
    fig = (abs(loss - ol) / ol, _rel(g_nn, og), _rel(g_t, ot))
    print(f"{tag} own steps: loss {fig[0]:.2e}  g_nn {fig[1]:.2e}  g_cond {fig[2]:.2e}")
    assert fig[0] <= 1e-8 and fig[1] <= 1e-6 and fig[2] <= 1e-6
    rec = ac.supp_solve(s, N - 1)[1]
    assert ac.same_steps(rec, *steps[N - 1], s["tp"][-1], 1e-6)


# ----------------------------------------------------------------------------- d: failing lanes on the one-body kernels
@pytest.mark.parametrize("kind", ["cpep", "supp"])
def test_lanes_that_fail_beside_lanes_that_go_on_in_the_one_body_kernels(kind):
    """tests/test_gpu_adaptive_grad.py test_lanes_that_fail_beside_lanes_that_go_on_in_a_gradient_launch for the kernels it
    does not reach: the one-body kernel of the c-peptide model (six knots, (2,6,3): the second translation unit) and of
    the suppression model ((4,4,2)), 70 subjects = one full wave and one of six lanes.  Subject 3 gets a NaN and subject
    66 a +Inf conditional parameter: the evaluation fails as the reference's does (loss +Inf, two failed subjects, their
    SSE non-finite), and every other subject's SSE, trajectory, accepted steps and conditional gradient are those of
    the clean run bit for bit."""
    from cude.engine import Engine
    N, bad = 70, [3, 66]
    if kind == "cpep":
        arch = (2, 6, 3)
        c = ac.cpep_case(arch, ac.CPEP_SHAPES.index(arch), ac.TP6, N)
        eng = Engine("cpep", arch, n_steps=0, n_state=2)
        eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
        nn, cond = c["nn"], c["beta"]
    else:
        s = ac.supp_case((4, 2), ac.SUPP_SHAPES.index((4, 2)), N)
        assert (4, 2) not in ac.SUPP_UNROLLED
        eng = Engine("supp", s["arch"], n_steps=0, lam=0.01)
        eng.set_population_supp(s["tp"], s["data"])
        nn, cond = s["nn"], s["theta"]
    runs = []
    for hit in (False, True):
        x = cond.copy()
        if hit:
            x[3], x[66] = np.nan, np.inf
        eng.set_params(nn, x)
        f = eng.forward(want_sse=True, want_traj=True)
        n_fwd = eng.n_failed()
        loss, g_nn, g_c = eng.loss_grad()
        steps = {i: eng.adaptive_steps(i) for i in range(N) if i not in bad}
        runs.append((f, n_fwd, loss, g_nn, g_c, eng.n_failed(), steps))
    eng.close()
    (f0, nf0, l0, gn0, gc0, ng0, st0), (f1, nf1, l1, gn1, gc1, ng1, st1) = runs
    assert np.isfinite(f0["loss"]) and np.isfinite(l0) and nf0 == 0 and ng0 == 0 and np.all(np.isfinite(gc0))
    assert f1["loss"] == np.inf and l1 == np.inf and nf1 == 2 and ng1 == 2
    assert not np.isfinite(f1["sse"][bad]).any()
    keep = np.setdiff1d(np.arange(N), bad)
    assert np.array_equal(f1["sse"][keep], f0["sse"][keep])
    assert np.array_equal(f1["traj"][:, :, keep], f0["traj"][:, :, keep])
    assert all(np.array_equal(st1[i][0], st0[i][0]) and np.array_equal(st1[i][1], st0[i][1]) for i in keep)
    assert np.array_equal(gc1[keep], gc0[keep]) and np.all(gc0[keep] != 0.0)


# ----------------------------------------------------------------------------- e: fixed step, live biases
@pytest.mark.parametrize("k", range(len(ac.CPEP_SHAPES)), ids=CPEP_IDS)
def test_cpep_fixed_step_with_live_biases(k):
    """The c-peptide leg of tests/test_gpu_parity.py test_every_compiled_shape_against_the_oracle -- the one-lane path
    and the time-split path against the C oracle, 30 steps -- on inputs whose biases are not zero."""
    import c_oracle as co
    from cude.engine import Engine
    arch = ac.CPEP_SHAPES[k]
    N, n_state = 66 + k, 2 + (k % 2)
    c = ac.cpep_case(arch, k, ac.TP5, N)
    # the forward-mode oracle carries at most 128 partials: the two largest shapes go to the reverse-mode one
    method = "forward" if c["nn"].size + 1 <= 128 else "reverse"
    ref = co.cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"], arch, c["nn"], c["beta"], 30, n_state,
                  covariate=(arch[0] == 3), method=method)
    for path in ("1", "2:3"):
        eng = Engine("cpep", arch, n_steps=30, n_state=n_state)
        eng.set_option("cpep_path", path)
        eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
        eng.set_params(c["nn"], c["beta"])
        loss, g_nn, g_cond = eng.loss_grad()
        eng.close()
        fig = (abs(loss - ref["loss"]) / abs(ref["loss"]), _rel(g_nn, ref["g_nn"]), _rel(g_cond, ref["g_beta"]))
        print(f"cpep fixed {arch} path {path}: loss {fig[0]:.2e}  g_nn {fig[1]:.2e}  g_cond {fig[2]:.2e}")
        assert fig[0] <= LOSS_RTOL and fig[1] < GRAD_RTOL and fig[2] < GRAD_RTOL, (arch, path)
        _blocks(f"cpep fixed {arch} path {path}", g_nn, ref["g_nn"], arch)


@pytest.mark.parametrize("k", range(len(ac.SUPP_SHAPES)), ids=SUPP_IDS)
def test_supp_fixed_step_with_live_biases(k):
    import c_oracle as co
    from cude.engine import Engine
    s = ac.supp_case(ac.SUPP_SHAPES[k], k, 40 + k)
    arch = s["arch"]
    ref = co.supp(s["tp"], s["data"], arch, s["nn"], s["theta"], 0.01, 30)
    eng = Engine("supp", arch, n_steps=30, lam=0.01)
    eng.set_population_supp(s["tp"], s["data"])
    eng.set_params(s["nn"], s["theta"])
    loss, g_nn, g_cond = eng.loss_grad()
    eng.close()
    fig = (abs(loss - ref["loss"]) / abs(ref["loss"]), _rel(g_nn, ref["g_nn"]), _rel(g_cond, ref["g_theta"]))
    print(f"supp fixed {arch}: loss {fig[0]:.2e}  g_nn {fig[1]:.2e}  g_cond {fig[2]:.2e}")
    assert fig[0] <= LOSS_RTOL and fig[1] < GRAD_RTOL and fig[2] < GRAD_RTOL, arch


# ----------------------------------------------------------------------------- the controller, over all shapes
def test_device_steps_are_the_oracles_over_all_shapes():
    """Over the 48 c-peptide cases of this module together: at least 90 % of the subjects take the oracle's own accepted
    steps (the bar of tests/test_gpu_adaptive_grad.py).  Reads what the per-shape tests computed (and computes it when run
    on its own)."""
    same = total = 0
    for grid in GRIDS:
        for k in range(len(ac.CPEP_SHAPES)):
            r = _cpep(grid, k)
            same, total = same + r["same"], total + r["N"]
    print(f"controller: {same} of {total} subjects take the oracle's steps")
    assert total == 2 * (21 * 16 + 3 * 70) and same >= math.ceil(0.9 * total), (same, total)
