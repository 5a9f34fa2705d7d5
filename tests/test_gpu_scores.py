"""cude_subject_scores on the device (the numbered rules in include/cude.h): the per-lane gradient rows the one-lane gradient
kernels leave behind, their fold over weighted sets, failures, the sum and cross product over the subjects, and the
mirrors built on them (api.marginal_score, api.train_marginal).

Bars.  Rows against the oracles: the project's own bars for the shared gradient against the same oracles -- fixed-step
1e-9 of the reference row's max-norm (tests/test_gpu_parity.py; torch autograd of sse[i], scores_ref.*_rows_torch),
adaptive 1e-8 of it against the replay of the accepted steps (tests/test_gpu_adaptive_grad.py:46; the oracle's
complex-step derivative of the step sequence, scores_ref.*_rows_replay on one-subject populations).  The sequence replayed
is the DEVICE's own, read with adaptive_steps behind a loss_grad call at the same parameters, as in that file: at the
solver's default tolerances two correct solvers do not always accept the same steps, and the 1e-8 bar is that of a replay
(the oracle's own sequences, cude_oracle.*_adaptive_loss_grad, agree at the solver's tolerance only).
A subject whose glucose never leaves its baseline has no production term at all: its reference row is exactly zero (subject
48 of conftest.make_cpep_case's 70), the device's is the rounding residue of terms that cancel -- the baseline evaluation
against the sum of the stage evaluations at the same input -- and a bar relative to zero says nothing.  Those terms are of
the size of the other subjects' rows (same network, same kinetics), so such a row is held to the same fraction of the
MEDIAN max-norm of the reference rows.
Rows against the shared gradient of the same kernels: |sum_i row_i[q] / N - g_nn[q]| <= 2^-50 (N + 64) sum_i |row_i[q]| / N
-- both sides add the same per-lane values in different orders, one more rounding per term from inv_n on the one side; four
times that worst case.  One entry has no such values: the bias of an IDENTITY output unit drops out of NN(x) - NN(0), its
gradient is identically zero, and what either side holds is the residue of weights that cancel (rounded before the
cancellation, at different scales: inv_n is 1 on one side, 1/N on the other).  The weights are those of the output
weights' columns, so for that entry the bar is formed with the largest column sum instead of its own.
Sum and cross product against math.fsum over the device's own score_out: 2^-52 (N + 4) sum_i |s_iq| |s_ir|, the forward
error bound of any order of summation, doubled.

Shapes: N = 70 (two workgroups, the second with six live lanes) and N = 5; P = 1 (the symbolic model) up to P = 193.  No
tuned shape has 193 parameters (the widest are the c-peptide 2-8-8-8-1 with 177 and the suppression 4-8-8-1 / 4-6-6-6-1
with 121): the suppression chain 4-8-8-8-1 = 193 runs on the fallback kernel, and the widest tuned shapes are run as well.

Not reachable from outside: CUDE_ERR_STATE under stream capture."""
import math

import numpy as np
import pytest
import torch  # noqa: F401  (first: shared HIP runtime)

import adaptive_cases as ac
import scores_ref as sr
from conftest import make_cpep_case, make_supp_case

pytestmark = pytest.mark.gpu

SYM_P0 = 1.78
CASES = ("cpep-2441", "cpep-2661", "cpep-3441", "supp-4355", "sym-log", "sym-raw", "cpep-2441-relu-identity",
         "fallback-2441", "fallback-chain")
_DATA = {}


def _case(name, N):
    """dict(model, arch of the engine, arch of the oracle, the case's arrays with nn / cond, cond_space, options, network)"""
    key = (name, N)
    if key in _DATA:
        return _DATA[key]
    d = dict(model="cpep", cond_space="log", options=(), network=None)
    if name == "supp-4355":
        c = make_supp_case(N, (4, 3, 5))
        d.update(model="supp", arch=(4, 3, 5), oarch=(4, 3, 5), c=c, cond=c["theta"])
    elif name.startswith("sym"):
        c = make_cpep_case(N, (2, 4, 2))
        raw = name == "sym-raw"
        k = 20.0 * (1.0 + 0.2 * np.random.default_rng(3).standard_normal(N))
        c = dict(c, nn=np.array([SYM_P0]))
        d.update(model="cpep_sym", arch=(1, 0, 0), oarch=(1, 0, 0), c=c, cond=k if raw else np.log(k),
                 cond_space="raw" if raw else "log")
    elif name == "cpep-3441":
        c = make_cpep_case(N, (3, 4, 2))
        nn = c["nn"].copy()
        nn[8:12] *= 0.02                          # (the raw age, 20 ... 79, is a network input: keep the units unsaturated)
        d.update(arch=(3, 4, 2), oarch=(3, 4, 2), c=dict(c, nn=nn), cond=c["beta"])
    elif name == "cpep-2441-relu-identity":
        c = make_cpep_case(N, (2, 4, 2))
        d.update(arch=(2, 4, 2), oarch=(2, 4, 2, "relu", "identity"), c=c, cond=c["beta"],
                 options=(("hidden_activation", "relu"), ("output_activation", "identity")))
    elif name == "fallback-2441":
        c = make_cpep_case(N, (2, 4, 2))
        d.update(arch=(2, 4, 2), oarch=(2, 4, 2), c=c, cond=c["beta"], options=(("force_fallback", 1),),
                 network=([4, 4], ["tanh", "tanh", "softplus"]))
    elif name == "fallback-chain":                # no tuned kernel has these widths
        import cude_oracle as o
        c = make_cpep_case(N, (2, 4, 2))
        arch = (2, (5, 3), ("tanh", "sigmoid"), "softplus")
        nn = 0.4 * np.random.default_rng(12).standard_normal(o.n_params(arch))
        d.update(arch=arch, oarch=arch, c=dict(c, nn=nn), cond=c["beta"])
    else:
        arch = {"cpep-2441": (2, 4, 2), "cpep-2661": (2, 6, 2)}[name]
        c = make_cpep_case(N, arch)
        d.update(arch=arch, oarch=arch, c=c, cond=c["beta"])
    d["cond"] = np.array(d["cond"], dtype=np.float64)
    _DATA[key] = d
    return d


def _engine(d, n_steps, options=()):
    from cude.engine import Engine
    if d["model"] == "supp":
        eng = Engine("supp", d["arch"], n_steps=n_steps)
    else:
        eng = Engine(d["model"], d["arch"], n_steps=n_steps, n_state=2, cond_space=d["cond_space"])
    for k, v in tuple(d["options"]) + tuple(options):
        eng.set_option(k, v)
    if d["network"] is not None:
        eng.set_network(*d["network"])
    assert eng.fallback_kernel == (d["network"] is not None or ac.o.general_arch(d["arch"]))
    c = d["c"]
    if d["model"] == "supp":
        eng.set_population_supp(c["tp"], c["data"])
    else:
        eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
    eng.set_params(c["nn"], d["cond"])
    return eng


def _reference_rows(d, eng, n_steps, cond=None):
    """(rows (N, P), sse (N,)) of the oracle at the conditionals `cond` (None: the case's)"""
    c = d["c"]
    if n_steps > 0:
        if d["model"] == "supp":
            return sr.supp_rows_torch(c, d["oarch"], cond, n_steps)
        return sr.cpep_rows_torch(dict(c, beta=d["cond"]), d["oarch"], cond, n_steps, d["cond_space"])
    x = d["cond"] if cond is None else cond
    eng.set_params(None, x)
    eng.loss_grad()
    steps = [list(zip(*eng.adaptive_steps(i))) for i in range(x.size)]
    eng.set_params(None, d["cond"])
    if d["model"] == "supp":
        return sr.supp_rows_replay(c, d["oarch"], steps, x)
    return sr.cpep_rows_replay(c, d["oarch"], steps, x, d["cond_space"])


def _same(tag, got, want, keys=("scores", "wsse", "bad", "sum", "cross"), subjects=None):
    for k in keys:
        g, w = got[k], want[k]
        if subjects is not None and k in ("scores", "wsse", "bad"):
            g, w = g[subjects], w[subjects]
        assert np.array_equal(g, w, equal_nan=True), (tag, k)


def _sets(d, K, seed=4):
    return d["cond"][None, :] + 0.05 * np.abs(d["cond"]).mean() * np.random.default_rng(seed).standard_normal((K, d["cond"].size))


# ---------------------------------------------------------------------------------------------- 1. rows against the oracles
@pytest.mark.parametrize("N", [70, 5])
@pytest.mark.parametrize("n_steps", [30, 0], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("name", CASES)
def test_rows_against_per_subject_oracle_gradients(name, n_steps, N):
    d = _case(name, N)
    eng = _engine(d, n_steps)
    want, want_sse = _reference_rows(d, eng, n_steps)
    got = eng.subject_scores()
    assert eng.n_failed() == 0 and not got["bad"].any()
    size = np.max(np.abs(want), axis=1)
    assert np.count_nonzero(size) >= 0.9 * N
    bar = (1e-9 if n_steps > 0 else 1e-8) * np.where(size > 0.0, size, np.median(size))     # (zero rows: the docstring)
    err = np.max(np.abs(got["scores"] - want), axis=1)
    print(f"{name} S={n_steps} N={N}: rows error / bar {np.max(err / np.maximum(bar, 1e-300)):.3g}, "
          f"sse {np.max(np.abs(got['wsse'] - want_sse) / want_sse):.3g}")
    assert np.all(err <= bar), (name, float(np.max(err / np.maximum(bar, 1e-300))))
    assert np.max(np.abs(got["wsse"] - want_sse)) <= 1e-10 * np.max(want_sse)        # one set, no weights: wsse is the SSE
    nn, cond = eng.get_params()
    assert np.array_equal(nn, d["c"]["nn"]) and np.array_equal(cond, d["cond"])      # the context's parameters are untouched
    # explicit conditionals: the same rows, bit for bit
    _same(name, eng.subject_scores(d["cond"][None, :]), got)
    if n_steps == 0:
        from cude._lib import CudeError
        with pytest.raises(CudeError):
            eng.adaptive_steps(0)
    eng.close()


# ------------------------------------------------------------------------ 2. every kernel that gained the epilogue
def _sum_against_shared_gradient(tag, eng, identity_output=False):
    """sum_i row_i / N against loss_grad on the same (one-lane) kernels"""
    N = eng.N
    _, g_nn, _ = eng.loss_grad()
    got = eng.subject_scores(want=("scores", "bad"))
    assert not got["bad"].any(), tag
    rows = got["scores"]
    col = np.abs(rows).sum(axis=0)
    if identity_output:                           # (the output bias: the docstring)
        assert col[-1] <= 1e-9 * col.max()
        col[-1] = col.max()
    bar = 2.0 ** -50 * (N + 64) * col / N
    err = np.abs(rows.sum(axis=0) / N - g_nn)
    assert np.all(err <= bar), (tag, float(np.max(err / np.maximum(bar, 1e-300))))
    assert np.max(np.abs(g_nn)) > 0.0, tag
    return float(np.max(err / np.maximum(bar, 1e-300)))


ONE_LANE = (("cpep_path", "1"), ("adaptive_team", 0), ("supp_store", 0))


def _run_shape(tag, model, arch, c, cond, n_steps, n_state=2, options=(), cond_space="log"):
    from cude.engine import Engine
    eng = Engine("supp", arch, n_steps=n_steps) if model == "supp" else \
        Engine(model, arch, n_steps=n_steps, n_state=n_state, cond_space=cond_space)
    for k, v in ONE_LANE + tuple(options):
        eng.set_option(k, v)
    assert not eng.fallback_kernel
    if model == "supp":
        eng.set_population_supp(c["tp"], c["data"])
    else:
        eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
    eng.set_params(c["nn"], cond)
    r = _sum_against_shared_gradient(tag, eng, model != "supp" and ("output_activation", "identity") in tuple(options))
    eng.close()
    return r


@pytest.mark.parametrize("group", [0, 1, 2])
def test_every_fixed_step_cpeptide_kernel(group):
    worst = 0.0
    for k, arch in list(enumerate(ac.CPEP_SHAPES))[8 * group:8 * group + 8]:
        c = make_cpep_case(ac.cpep_subjects(arch), arch)
        nn = c["nn"].copy()
        if arch[0] == 3:
            nn[2 * arch[1]:3 * arch[1]] *= 0.02
        for n_state in (2, 3):
            worst = max(worst, _run_shape((arch, n_state), "cpep", arch, dict(c, nn=nn), c["beta"], 30, n_state))
    print(f"fixed-step c-peptide shapes, group {group}: largest error / bar {worst:.3g}")


@pytest.mark.parametrize("tp", [ac.TP5, ac.TP6], ids=["unrolled", "one-body"])
@pytest.mark.parametrize("group", [0, 1, 2])
def test_every_adaptive_cpeptide_kernel(group, tp):
    worst = 0.0
    for k, arch in list(enumerate(ac.CPEP_SHAPES))[8 * group:8 * group + 8]:
        c = ac.cpep_case(arch, k, tp, ac.cpep_subjects(arch))
        worst = max(worst, _run_shape((arch, len(tp)), "cpep", arch, c, c["beta"], 0))
    print(f"adaptive c-peptide shapes, group {group}, {len(tp)} knots: largest error / bar {worst:.3g}")


@pytest.mark.parametrize("n_steps", [30, 0], ids=["fixed", "adaptive"])
def test_every_suppression_kernel(n_steps):
    worst = 0.0
    for k, shape in enumerate(ac.SUPP_SHAPES):
        s = ac.supp_case(shape, k, 70 if k % 5 == 0 else 16)
        worst = max(worst, _run_shape((shape, n_steps), "supp", s["arch"], s, s["theta"], n_steps))
    print(f"suppression shapes, S={n_steps}: largest error / bar {worst:.3g}")


@pytest.mark.parametrize("n_steps", [30, 0], ids=["fixed", "adaptive"])
def test_every_general_activation_and_symbolic_kernel(n_steps):
    from test_gpu_activations import COMBOS
    worst = 0.0
    for arch in ((2, 4, 2), (2, 6, 2), (3, 4, 2)):
        for tp in ((ac.TP5, ac.TP6) if n_steps == 0 else (ac.TP5,)):      # (adaptive: these shapes run the one-body kernel)
            c = ac.cpep_case(arch, 3, tp, 70 if arch == (2, 4, 2) else 16)
            for hidden, output in COMBOS:
                opts = (("hidden_activation", hidden), ("output_activation", output))
                worst = max(worst, _run_shape((arch, hidden, output), "cpep", arch, c, c["beta"], n_steps, options=opts))
    for shape in ((3, 5), (3, 3)):
        s = ac.supp_case(shape, 1, 16)
        for hidden, output in COMBOS:
            opts = (("hidden_activation", hidden), ("output_activation", output))
            worst = max(worst, _run_shape((shape, hidden, output), "supp", s["arch"], s, s["theta"], n_steps, options=opts))
    for space in ("log", "raw"):                  # the symbolic model: unrolled (five knots) and one-body (six) when adaptive
        for tp in ((ac.TP5, ac.TP6) if n_steps == 0 else (ac.TP5,)):
            c = ac.cpep_case((2, 4, 2), 0, tp, 70)
            k = 20.0 * (1.0 + 0.2 * np.random.default_rng(3).standard_normal(70))
            worst = max(worst, _run_shape(("sym", space, len(tp)), "cpep_sym", (1, 0, 0), dict(c, nn=np.array([SYM_P0])),
                                          k if space == "raw" else np.log(k), n_steps, cond_space=space))
    print(f"general-activation and symbolic kernels, S={n_steps}: largest error / bar {worst:.3g}")


# ---------------------------------------------------------------------------------------------------------------- 3. fold
FOLD = [("cpep-2441", 30), ("cpep-2441", 0), ("supp-4355", 30), ("supp-4355", 0), ("fallback-2441", 30), ("sym-raw", 30)]


@pytest.mark.parametrize("name,n_steps", FOLD)
def test_fold_equals_the_restatement_for_every_chunking(name, n_steps):
    d = _case(name, 70)
    K = 5
    sets = _sets(d, K)
    rng = np.random.default_rng(21)
    w = rng.standard_normal((K, 70))              # both signs
    w[rng.random((K, 70)) < 0.1] = 0.0
    eng = _engine(d, n_steps)
    single = [eng.subject_scores(sets[k:k + 1]) for k in range(K)]
    assert all(not s["bad"].any() for s in single)
    s, ws, bad = sr.fold(np.stack([r["scores"] for r in single]), np.stack([r["wsse"] for r in single]), w)
    want_scores, want_wsse, failed = sr.finish(s, ws, bad)
    assert not failed.any()
    got = eng.subject_scores(sets, w)
    assert np.array_equal(got["scores"], want_scores) and np.array_equal(got["wsse"], want_wsse) and not got["bad"].any()
    # weights None = 1
    s1, ws1, _ = sr.fold(np.stack([r["scores"] for r in single]), np.stack([r["wsse"] for r in single]))
    ones = eng.subject_scores(sets)
    assert np.array_equal(ones["scores"], s1) and np.array_equal(ones["wsse"], ws1)
    _same(name, eng.subject_scores(sets, np.ones((K, 70))), ones)
    eng.close()
    for chunk in (0, 1, 2, 5):
        e2 = _engine(d, n_steps, options=(("profile_chunk", chunk),))
        _same((name, chunk), e2.subject_scores(sets, w), got)
        e2.close()


# ------------------------------------------------------------------------------------------ 4. zero weight and failures
@pytest.mark.parametrize("name,n_steps", FOLD)
def test_zero_weight_skips_and_a_failure_marks_its_subject_only(name, n_steps):
    d = _case(name, 70)
    K, bad_set, bad_subject = 4, 2, 11
    sets = _sets(d, K, seed=6)
    w = 0.5 + np.random.default_rng(22).random((K, 70))
    eng = _engine(d, n_steps)
    clean = eng.subject_scores(np.delete(sets, bad_set, axis=0), np.delete(w, bad_set, axis=0))
    poisoned = sets.copy()
    poisoned[bad_set, bad_subject] = np.nan
    # weight 0 on the bad node: as if the set were not there for that subject -- and with the whole set at weight 0, for all
    w0 = w.copy()
    w0[bad_set, :] = 0.0
    _same(name, eng.subject_scores(poisoned, w0), clean)
    assert eng.n_failed() == 0
    # weight 1: that subject fails, alone
    w1 = w.copy()
    w1[bad_set, bad_subject] = 1.0
    got = eng.subject_scores(poisoned, w1)
    assert eng.n_failed() == 1
    full = eng.subject_scores(sets, w1)
    assert eng.n_failed() == 0
    others = np.arange(70) != bad_subject
    assert np.isnan(got["scores"][bad_subject]).all() and np.isnan(got["wsse"][bad_subject])
    assert got["bad"][bad_subject] == 1 and not got["bad"][others].any()
    _same(name, got, full, keys=("scores", "wsse", "bad"), subjects=others)
    # sum / cross: the other subjects' values alone -- the call in which that subject has no weight at all (its row is 0)
    w_out = w1.copy()
    w_out[:, bad_subject] = 0.0
    without = eng.subject_scores(sets, w_out)
    assert np.all(without["scores"][bad_subject] == 0.0)
    _same(name, got, without, keys=("sum", "cross"))
    assert np.isfinite(got["sum"]).all() and np.isfinite(got["cross"]).all()
    eng.close()


# ------------------------------------------------------------------------------------------------------ 5. sum and cross
def _check_sum_cross(tag, got, N, mask=None):
    scores = got["scores"]
    tot, cross, asum, across = sr.exact_sum_cross(scores)
    u = 2.0 ** -52 * (N + 4)
    assert np.all(np.abs(got["sum"] - tot) <= u * asum), tag
    assert np.all(np.abs(got["cross"] - cross) <= u * across), tag
    assert np.array_equal(got["cross"], got["cross"].T), tag
    if mask is not None:
        off = np.asarray(mask) == 0.0
        assert np.all(scores[:, off] == 0.0) and np.all(got["sum"][off] == 0.0), tag
        assert np.all(got["cross"][off, :] == 0.0) and np.all(got["cross"][:, off] == 0.0), tag
        assert np.all(np.signbit(scores[:, off]) == False) and np.all(np.signbit(got["sum"][off]) == False), tag  # noqa: E712
    r = np.abs(got["cross"] - cross) / np.maximum(u * across, 1e-300)
    return float(np.max(r))


@pytest.mark.parametrize("n_steps", [30, 0], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("name", ["cpep-2441", "cpep-2661", "supp-4355", "sym-raw", "sym-log"])
def test_sum_and_cross_product(name, n_steps):
    for N in (70, 5):
        d = _case(name, N)
        eng = _engine(d, n_steps)
        K = 3
        sets, w = _sets(d, K, seed=8), np.random.default_rng(23).standard_normal((K, N))
        got = eng.subject_scores(sets, w)
        worst = _check_sum_cross((name, N), got, N)
        # ... asked for alone: the same numbers (the host never needs the table)
        alone = eng.subject_scores(sets, w, want=("sum", "cross"))
        assert alone["scores"] is None and np.array_equal(alone["sum"], got["sum"]) and np.array_equal(alone["cross"], got["cross"])
        again = eng.subject_scores(sets, w)
        _same(name, again, got)                   # the same from run to run
        if eng.P > 1:
            mask = np.ones(eng.P)
            mask[[0, eng.P // 2, eng.P - 1]] = 0.0
            eng.set_param_mask(mask)
            masked = eng.subject_scores(sets, w)
            _check_sum_cross((name, N, "mask"), masked, N, mask)
            on = mask == 1.0
            assert np.array_equal(masked["scores"][:, on], got["scores"][:, on])
            # a failed subject's row: NaN, masked entries still exactly 0
            bad = sets.copy()
            bad[1, 2] = np.nan
            wb = np.abs(w) + 0.1
            f = eng.subject_scores(bad, wb)
            assert np.isnan(f["scores"][2, on]).all() and np.all(f["scores"][2, ~on] == 0.0)
            _check_sum_cross((name, N, "mask+fail"), f, N, mask)
            eng.set_param_mask(None)
        print(f"{name} S={n_steps} N={N}: cross error / bar {worst:.3g}")
        eng.close()


def test_sum_and_cross_product_at_the_widest_shapes():
    """P = 193 (suppression 4-8-8-8-1, the fallback kernel), and the widest tuned shapes: suppression 4-8-8-1 (P = 121) and
    c-peptide 2-8-8-8-1 (P = 177); N = 70"""
    from cude.engine import Engine
    import cude_oracle as o
    N = 70
    s = make_supp_case(N, (4, 3, 5))
    for arch, fallback in (((4, (8, 8, 8), "tanh", "softplus"), True), ((4, 8, 2), False)):
        eng = Engine("supp", arch, n_steps=30)
        assert eng.fallback_kernel == fallback and eng.P == (193 if fallback else 121)
        eng.set_population_supp(s["tp"], s["data"])
        nn = ac.biased_params((4, 8, 2), 5) if not fallback else 0.3 * np.random.default_rng(5).standard_normal(193)
        eng.set_params(nn, s["theta"])
        got = eng.subject_scores()
        assert not got["bad"].any() and np.count_nonzero(got["scores"]) > 0.9 * got["scores"].size
        print(f"P = {eng.P}: cross error / bar {_check_sum_cross(arch, got, N):.3g}")
        eng.close()
    c = make_cpep_case(N, (2, 8, 3))
    eng = Engine("cpep", (2, 8, 3), n_steps=30, n_state=2)
    assert not eng.fallback_kernel and eng.P == 177 == o.n_params((2, 8, 3))
    eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
    eng.set_params(c["nn"], c["beta"])
    got = eng.subject_scores()
    print(f"P = 177: cross error / bar {_check_sum_cross((2, 8, 3), got, N):.3g}")
    eng.close()


# ------------------------------------------------------------------------------------------------------------ 6. regroup
def test_regrouped_launch_gives_the_same_rows():
    """adaptive mode, 8262 subjects (129 full waves and one of six lanes): with auto_regroup the second call runs in the
    order of the first one's accepted-step counts; score_out does not depend on it"""
    N = 8262
    base = make_cpep_case(70, (2, 4, 2))
    idx = np.arange(N) % 70
    rng = np.random.default_rng(31)
    c = {k: (base[k][idx] if k in ("G", "obs", "age", "t2dm") else base[k]) for k in ("tp", "G", "obs", "age", "t2dm", "nn")}
    cond = base["beta"][idx] + 0.5 * rng.standard_normal(N)      # (a spread of step counts to sort by)
    d = dict(model="cpep", arch=(2, 4, 2), cond_space="log", options=(), network=None, c=c, cond=cond)
    tables = []
    for auto in (1, 0):
        eng = _engine(d, 0, options=(("auto_regroup", auto),))
        eng.subject_scores(want=("wsse",))        # the first call leaves the counts the second one is ordered by
        tables.append(eng.subject_scores())
        before, after = eng.adaptive_regroup()    # (auto: that call already ran in the sorted order)
        assert before == after if auto else after < before
        eng.close()
    _same("regroup", tables[0], tables[1], keys=("scores", "wsse", "bad"))
    assert np.isfinite(tables[0]["scores"]).all()


# --------------------------------------------------------------------------------------------------------- 7. end to end
def test_marginal_score_against_the_oracles_autograd():
    """fixed-step 2-4-4-1, N = 5, K = 5, explicit centres and scales, sigma = sqrt(median SSE / T): api.marginal_score's
    gradient against torch autograd of sum_i logsumexp_k t_ik through the oracle.  Bar: (1e-9 + 1e-10 max_ik SSE_ik / (2
    sigma^2)) max_q sum_i sum_k w_ik |row_ik[q]| / (2 sigma^2) -- the gradient bar plus the SSE bar carried through the
    weights."""
    from cude import api
    import test_gpu_predictive as tgp
    arch, N, K = (2, 4, 2), 5, 5
    c = make_cpep_case(N, arch)
    pm, sd = -0.6, 0.9
    rng = np.random.default_rng(7)
    center, scale = c["beta"] + 0.1 * rng.standard_normal(N), 0.05 + 0.3 * rng.random(N)
    z, a = api.gauss_hermite_rule(K)
    points = center[None, :] + scale[None, :] * z[:, None]
    sigma = float(np.sqrt(np.median(sr.cpep_rows_torch(c, arch)[1]) / len(c["tp"])))
    m = sr.marginal_cpep_torch(c, arch, points, a, sigma, pm, sd)
    models = tgp._api_models(api, c, arch, N)
    try:
        ms = api.marginal_score(None, c["nn"], models, c["tp"], c["obs"], sigma, pm, sd, method="quadrature", n_nodes=K,
                                n_steps=30, center=center, scale=scale)
        se = api.network_standard_errors(None, c["nn"], models, c["tp"], c["obs"], sigma, pm, sd, method="quadrature",
                                         n_nodes=K, n_steps=30, center=center, scale=scale)
        table = api.subject_scores(api.ComponentArray(neural=c["nn"], conditional=c["beta"][:, None]), (models, c["tp"], c["obs"]),
                                   n_steps=30)
    finally:
        api.clear_cache()
    c2 = 1.0 / (2.0 * sigma * sigma)
    bar = (1e-9 + 1e-10 * np.max(m["sse"]) * c2) * np.max(np.einsum("kn,knp->p", m["w"], np.abs(m["rows"]))) * c2
    err = np.max(np.abs(ms.gradient - m["gradient"]))
    print(f"marginal gradient: error {err:.3g}, bar {bar:.3g}, total {ms.total:.12g} against {m['total']:.12g}")
    assert err <= bar and ms.n_failed == 0
    assert abs(ms.total - (m["total"] + np.log(scale).sum())) <= 1e-9 * abs(m["total"])
    # every subject's own gradient, and the OPG matrix built from them
    own = -c2 * np.einsum("kn,knp->np", m["w"], m["rows"])
    assert np.max(np.abs(ms.scores - own)) <= bar
    assert np.allclose(ms.opg, ms.scores.T @ ms.scores, rtol=1e-12, atol=1e-12 * np.max(np.abs(ms.opg)))
    assert np.array_equal(ms.opg, ms.opg.T) and se.rank <= N and np.array_equal(se.opg, ms.opg)
    assert se.se.shape == (c["nn"].size,) and np.isfinite(se.se).all()
    # wsse with these weights is the posterior expectation of the SSE: post_sse of the same call, within that file's bar
    B = 2.0 ** -50 * (K + np.max(np.abs(m["terms"]), axis=0) + np.abs(np.log(scale)) + 8)
    assert np.all(np.abs(ms.wsse - ms.post_sse) <= B * np.abs(ms.post_sse))
    # the K = 1 table of the mirror: the rows at the fitted conditionals
    want, _ = sr.cpep_rows_torch(c, arch)
    assert np.all(want.any(axis=1)) and np.all(np.max(np.abs(table - want), axis=1) <= 1e-9 * np.max(np.abs(want), axis=1))


# -------------------------------------------------------------------------------------------------------------- 8. errors
def test_argument_and_state_errors():
    from cude._lib import CudeError, check
    from cude.engine import Engine
    d = _case("cpep-2441", 5)
    eng = _engine(d, 30)
    lib, h = eng._lib, eng._h
    out = np.empty(5)

    def raw(n_sets, cond, w, wsse):
        p = lambda a: None if a is None else a.ctypes.data                       # noqa: E731
        check(lib.cude_subject_scores(h, n_sets, p(cond), p(w), None, p(wsse), None, None, None))

    with pytest.raises(CudeError, match="n_sets must be >= 1") as ei:
        raw(0, np.zeros((1, 5)), None, out)
    assert ei.value.status == -1
    with pytest.raises(CudeError, match="cond_sets is NULL with n_sets > 1") as ei:
        raw(2, None, None, out)
    assert ei.value.status == -1
    for v in (np.nan, np.inf, -np.inf):
        w = np.ones((2, 5))
        w[1, 3] = v
        with pytest.raises(CudeError, match="weights must be finite") as ei:
            eng.subject_scores(_sets(d, 2), w)
        assert ei.value.status == -1
    with pytest.raises(CudeError, match="no output requested") as ei:
        eng.subject_scores(want=())
    assert ei.value.status == -1
    with pytest.raises(ValueError):
        eng.subject_scores(np.zeros((2, 4)))
    with pytest.raises(ValueError):
        eng.subject_scores(_sets(d, 2), np.ones((3, 5)))
    raw(1, None, None, out)                       # NULL with one set: the context's conditionals
    assert np.array_equal(out, eng.subject_scores(want=("wsse",))["wsse"])
    eng.close()
    # state
    c = d["c"]
    eng = Engine("cpep", (2, 4, 2), n_steps=30, n_state=2)
    eng.N = 5
    with pytest.raises(CudeError, match="population not set") as ei:
        eng.subject_scores()
    state = ei.value.status
    assert state == -3
    eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
    with pytest.raises(CudeError, match="shared parameters not set") as ei:
        eng.subject_scores()
    assert ei.value.status == state
    eng.set_params(c["nn"], None)
    with pytest.raises(CudeError, match="conditional parameters are not set") as ei:
        eng.subject_scores()
    assert ei.value.status == state
    got = eng.subject_scores(d["cond"][None, :])  # explicit sets need none
    assert np.isfinite(got["scores"]).all()
    eng.close()


# ------------------------------------------------------------------------------------------------------ 9. train_marginal
def test_train_marginal_raises_the_marginal_likelihood():
    from cude import api
    import test_gpu_predictive as tgp
    arch, N = (2, 4, 2), 12
    c = make_cpep_case(N, arch)
    models = tgp._api_models(api, c, arch, N)
    sigma = float(np.sqrt(np.median(sr.cpep_rows_torch(c, arch)[1]) / len(c["tp"])))
    try:
        fit = api.train_marginal(c["nn"], models, c["tp"], c["obs"], sigma, -0.6, 0.9, rounds=1, iterations=5, method="grid",
                                 n_nodes=17, n_steps=30)
    finally:
        api.clear_cache()
    t = fit.trace
    print("train_marginal: total", t)
    assert 2 <= len(t) <= 6 and all(np.isfinite(t))
    assert all(b >= a for a, b in zip(t, t[1:])) and t[-1] > t[0]
    assert fit.nn.shape == c["nn"].shape and not np.array_equal(fit.nn, c["nn"])
    assert fit.sigma > 0 and fit.omega > 0 and math.isfinite(fit.prior_mean)
