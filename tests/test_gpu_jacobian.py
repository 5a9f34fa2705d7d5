"""cude_network_information on the device (the numbered rules in include/cude.h): the unit-seeded rows of the one-lane gradient
kernels (J_io = d yhat_io / d theta, jc_io = d yhat_io / d cond_i), their fold into b_i and d_i, failures and flat subjects, the
expected-information matrix A, its Schur complement S, the quadratic forms, and the mirrors built on them.

Bars.  Rows against the oracles: the bars and the reasoning of tests/test_gpu_scores.py's docstring -- fixed-step 1e-9 of the
reference row's max-norm against torch autograd of the oracle's trajectories (jacobian_ref.*_jac_torch), adaptive 1e-8 of it
against the complex-step derivative of the replay of the DEVICE's own accepted steps (jacobian_ref.*_jac_replay).  A row is
J_io (P entries); jc is held per subject, to the max-norm of its (n_out,) vector.  A subject whose glucose never leaves its
baseline (subject 48 of conftest.make_cpep_case's 70) has exactly-zero reference rows, the device's are the rounding residue of
terms that cancel: such a row is held to the same fraction of the MEDIAN max-norm of the live reference rows, as that file
does.  The rows of t_0 and of suppression state 0 are not computed at all: exactly +0.0.
Three checks the device makes on itself, at the same 1e-9 / 1e-8: jcond against cude_sensitivity's sens (independent tangent
kernels), dcond against that call's info, and sum_o 2 w_o r_io J_io (r from cude_forward's traj) against cude_subject_scores'
row.  Largest error / bar measured (MI355X, N = 70, all cases): jcond against sens 2.2e-3, dcond against info 3.0e-4, the
score rows 1.8e-4; rows against the oracles 5.4e-4, jc 2.2e-3.
A against math.fsum over the device's own jac_out: 2^-52 (N n_out + 4) sum |w J J|, the forward error bound of any order of
summation, doubled.  S: that plus 2^-50 (N + 4) sum_i |t_iq| |t_ir| for the Schur term (the square root and the division of
t_i = b_i / sqrt(d_i + pw) add roundings the exact form b b^T / (d + pw) does not have).  qform against numpy on the device's
own tables: 2^-52 (2 P + 8) sum_qr |z_q| |C_qr| |z_r|, two nested dot products of length P, doubled; z itself is formed from
the device's tables by the device's rule (product rounded, then the difference), so it is reproduced bit for bit.

Shapes: N = 70 (two workgroups, the second with six live lanes) and N = 5.

Not reachable from outside: CUDE_ERR_STATE under stream capture."""
import numpy as np
import pytest
import torch  # noqa: F401  (first: shared HIP runtime)

import adaptive_cases as ac
import jacobian_ref as jr
from conftest import make_cpep_case, make_supp_case
from test_gpu_scores import CASES as SCORE_CASES, ONE_LANE, SYM_P0, _case as _score_case

pytestmark = pytest.mark.gpu

CASES = SCORE_CASES + ("cpep-2441-ns3",)
# (case, n_steps): fixed-step (30) and adaptive (0); the adaptive mode integrates the 2-state c-peptide model only
CASE_MODES = [(n, s) for n in CASES for s in (30, 0) if not (n == "cpep-2441-ns3" and s == 0)]
ALL = ("jac", "jcond", "gn", "coupling", "dcond", "schur", "status")
_REF = {}


def _case(name, N):
    d = dict(_score_case("cpep-2441" if name == "cpep-2441-ns3" else name, N))
    d["n_state"] = 3 if name == "cpep-2441-ns3" else 2
    return d


def _engine(d, n_steps, options=()):
    from cude.engine import Engine
    if d["model"] == "supp":
        eng = Engine("supp", d["arch"], n_steps=n_steps)
    else:
        eng = Engine(d["model"], d["arch"], n_steps=n_steps, n_state=d["n_state"], cond_space=d["cond_space"])
    for k, v in tuple(d["options"]) + tuple(options):
        eng.set_option(k, v)
    if d["network"] is not None:
        eng.set_network(*d["network"])
    c = d["c"]
    if d["model"] == "supp":
        eng.set_population_supp(c["tp"], c["data"])
    else:
        eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
    eng.set_params(c["nn"], d["cond"])
    return eng


def _weights(d):
    c = d["c"]
    return jr.out_weights(d["model"], len(c["tp"]), c.get("data"))


def _reference(name, N, n_steps, eng):
    """(jac, jcond) of the oracle, computed once per case"""
    key = (name, N, n_steps)
    if key in _REF:
        return _REF[key]
    d = _case(name, N)
    c = d["c"]
    if n_steps > 0:
        if d["model"] == "supp":
            ref = jr.supp_jac_torch(c, d["oarch"], d["cond"], n_steps)
        else:
            ref = jr.cpep_jac_torch(c, d["oarch"], d["cond"], n_steps, d["cond_space"], d["n_state"])
    else:
        eng.loss_grad()
        steps = [list(zip(*eng.adaptive_steps(i))) for i in range(N)]
        if d["model"] == "supp":
            ref = jr.supp_jac_replay(c, d["oarch"], steps, d["cond"])
        else:
            ref = jr.cpep_jac_replay(c, d["oarch"], steps, d["cond"], d["cond_space"])
    _REF[key] = ref[:2]
    return _REF[key]


def _row_bar(want, tol):
    """tol x the max-norm of every reference row over its last axis; zero rows: the median of the others (the docstring).
    The flat subject's reference jc is not exactly zero but the reference's own residue of the same cancellation (autograd adds
    the baseline's term to the stages' terms: 1e-17 where the others are 1e-1): a row below 2^-30 of the median counts as zero."""
    size = np.max(np.abs(want), axis=-1)
    med = np.median(size[size > 0.0])
    live = size > 2.0 ** -30 * med
    return tol * np.where(live, size, np.median(size[live]))


def _dead_outputs(d):
    T = len(d["c"]["tp"])
    n_out = 3 * T if d["model"] == "supp" else T
    return sorted(set(range(n_out)) - set(jr.live_outputs(d["model"], T)))


# ---------------------------------------------------------------------------------------------- 1. rows against the oracles
@pytest.mark.parametrize("N", [70, 5])
@pytest.mark.parametrize("name,n_steps", CASE_MODES)
def test_rows_against_the_oracle_jacobian(name, n_steps, N):
    d = _case(name, N)
    eng = _engine(d, n_steps)
    want_j, want_c = _reference(name, N, n_steps, eng)
    got = eng.network_information(want=ALL)
    assert eng.n_failed() == 0 and not (got["status"] & jr.FAILED).any()
    assert eng.n_outputs == want_j.shape[1]
    tol = 1e-9 if n_steps > 0 else 1e-8
    live = jr.live_outputs(d["model"], len(d["c"]["tp"]))
    dead = _dead_outputs(d)
    bar = _row_bar(want_j[:, live], tol)
    err = np.max(np.abs(got["jac"][:, live] - want_j[:, live]), axis=-1)
    cbar = _row_bar(want_c, tol)
    cerr = np.max(np.abs(got["jcond"] - want_c), axis=-1)
    print(f"{name} S={n_steps} N={N}: rows error / bar {np.max(err / bar):.3g}, jc error / bar {np.max(cerr / cbar):.3g}")
    assert np.count_nonzero(np.max(np.abs(want_j[:, live]), axis=-1)) >= 0.9 * N * len(live)
    assert np.all(err <= bar), (name, float(np.max(err / bar)))
    assert np.all(cerr <= cbar), (name, float(np.max(cerr / cbar)))
    for k in ("jac", "jcond"):                    # t_0 and suppression state 0: exactly +0.0
        z = got[k][:, dead]
        assert np.all(z == 0.0) and not np.signbit(z).any(), (name, k)
    nn, cond = eng.get_params()
    assert np.array_equal(nn, d["c"]["nn"]) and np.array_equal(cond, d["cond"])      # the context's parameters are untouched
    again = eng.network_information(cond=d["cond"], want=ALL)                        # explicit conditionals: bit for bit
    for k in ALL:
        assert np.array_equal(got[k], again[k], equal_nan=True), (name, k)
    if n_steps == 0:
        from cude._lib import CudeError
        with pytest.raises(CudeError):
            eng.adaptive_steps(0)
    eng.close()


# ------------------------------------------------------------------------------- 2. three checks the device makes on itself
def _scores_from_jacobian(eng, d, got):
    """sum_o 2 w_o r_io J_io with r from cude_forward's traj -> (N, P)"""
    c = d["c"]
    traj = eng.forward(want_traj=True)["traj"]                     # (n_state, T, N)
    if d["model"] == "supp":
        r = (traj - c["data"]).transpose(2, 1, 0).reshape(eng.N, -1)              # (N, T, 3) -> o = s + 3 j
    else:
        r = (traj[0] - np.asarray(c["obs"]).T).T
    return 2.0 * np.einsum("o,io,iop->ip", _weights(d), r, got["jac"])


def _third_check(tag, eng, d, tol):
    got = eng.network_information(want=("jac", "status"))
    assert not (got["status"] & jr.FAILED).any(), tag
    mine = _scores_from_jacobian(eng, d, got)
    rows = eng.subject_scores(want=("scores",))["scores"]
    bar = _row_bar(rows, tol)
    err = np.max(np.abs(mine - rows), axis=1)
    assert np.all(err <= bar), (tag, float(np.max(err / bar)))
    assert np.max(np.abs(rows)) > 0.0, tag
    return float(np.max(err / bar))


@pytest.mark.parametrize("name,n_steps", CASE_MODES)
def test_device_checks_itself(name, n_steps):
    N = 70
    d = _case(name, N)
    eng = _engine(d, n_steps)
    tol = 1e-9 if n_steps > 0 else 1e-8
    r3 = _third_check(name, eng, d, tol)
    r1 = r2 = float("nan")
    if not eng.fallback_kernel:                   # (cude_sensitivity has no tangent solve on the fallback kernel)
        got = eng.network_information(want=("jcond", "dcond"))
        s = eng.sensitivity()
        sens = s["sens"]                          # (n_state, T, N)
        want_c = sens.transpose(2, 1, 0).reshape(N, -1) if d["model"] == "supp" else sens[0].T
        cbar = _row_bar(want_c, tol)
        cerr = np.max(np.abs(got["jcond"] - want_c), axis=1)
        assert np.all(cerr <= cbar), (name, float(np.max(cerr / cbar)))
        ibar = _row_bar(s["info"][:, None], tol)
        ierr = np.abs(got["dcond"] - s["info"])
        assert np.all(ierr <= ibar), (name, float(np.max(ierr / ibar)))
        r1, r2 = float(np.max(cerr / cbar)), float(np.max(ierr / ibar))
    print(f"{name} S={n_steps}: jcond/sens {r1:.3g}, dcond/info {r2:.3g}, scores {r3:.3g} (error / bar)")
    eng.close()


# ------------------------------------------------------------------------------ 3. every kernel that gained the unit seed
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
    r = _third_check(tag, eng, dict(model=model, c=c), 1e-9 if n_steps > 0 else 1e-8)
    eng.close()
    return r


@pytest.mark.parametrize("group", [0, 1, 2])
def test_every_fixed_step_cpeptide_kernel(group):
    worst = 0.0
    for k, arch in list(enumerate(ac.CPEP_SHAPES))[8 * group:8 * group + 8]:
        c = make_cpep_case(5, arch)
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
        c = ac.cpep_case(arch, k, tp, 5)
        worst = max(worst, _run_shape((arch, len(tp)), "cpep", arch, c, c["beta"], 0))
    print(f"adaptive c-peptide shapes, group {group}, {len(tp)} knots: largest error / bar {worst:.3g}")


@pytest.mark.parametrize("n_steps", [30, 0], ids=["fixed", "adaptive"])
def test_every_suppression_kernel(n_steps):
    worst = 0.0
    for k, shape in enumerate(ac.SUPP_SHAPES):
        s = ac.supp_case(shape, k, 5)
        worst = max(worst, _run_shape((shape, n_steps), "supp", s["arch"], s, s["theta"], n_steps))
    print(f"suppression shapes, S={n_steps}: largest error / bar {worst:.3g}")


@pytest.mark.parametrize("n_steps", [30, 0], ids=["fixed", "adaptive"])
def test_every_general_activation_and_symbolic_kernel(n_steps):
    from test_gpu_activations import COMBOS
    worst = 0.0
    for arch in ((2, 4, 2), (2, 6, 2), (3, 4, 2)):
        for tp in ((ac.TP5, ac.TP6) if n_steps == 0 else (ac.TP5,)):      # (adaptive: these shapes run the one-body kernel)
            c = ac.cpep_case(arch, 3, tp, 5)
            for hidden, output in COMBOS:
                opts = (("hidden_activation", hidden), ("output_activation", output))
                worst = max(worst, _run_shape((arch, hidden, output), "cpep", arch, c, c["beta"], n_steps, options=opts))
    for shape in ((3, 5), (3, 3)):
        s = ac.supp_case(shape, 1, 5)
        for hidden, output in COMBOS:
            opts = (("hidden_activation", hidden), ("output_activation", output))
            worst = max(worst, _run_shape((shape, hidden, output), "supp", s["arch"], s, s["theta"], n_steps, options=opts))
    for space in ("log", "raw"):                  # the symbolic model: unrolled (five knots) and one-body (six) when adaptive
        for tp in ((ac.TP5, ac.TP6) if n_steps == 0 else (ac.TP5,)):
            c = ac.cpep_case((2, 4, 2), 0, tp, 5)
            k = 20.0 * (1.0 + 0.2 * np.random.default_rng(3).standard_normal(5))
            worst = max(worst, _run_shape(("sym", space, len(tp)), "cpep_sym", (1, 0, 0), dict(c, nn=np.array([SYM_P0])),
                                          k if space == "raw" else np.log(k), n_steps, cond_space=space))
    print(f"general-activation and symbolic kernels, S={n_steps}: largest error / bar {worst:.3g}")


# ------------------------------------------------------------------------------------------------------------- 4. A and S
def _check_gn_schur(tag, got, w, pw, mask=None):
    N, n_out, P = got["jac"].shape
    A, mag = jr.exact_gn(got["jac"], w, got["status"])
    X, tmag = jr.exact_schur_term(got["coupling"], got["dcond"], pw, got["status"])
    abar = 2.0 ** -52 * (N * n_out + 4) * mag
    sbar = abar + 2.0 ** -50 * (N + 4) * tmag
    aerr, serr = np.abs(got["gn"] - A), np.abs(got["schur"] - (A - X))
    assert np.all(aerr <= abar), (tag, float(np.max(aerr / np.maximum(abar, 1e-300))))
    assert np.all(serr <= sbar), (tag, float(np.max(serr / np.maximum(sbar, 1e-300))))
    assert np.array_equal(got["gn"], got["gn"].T) and np.array_equal(got["schur"], got["schur"].T), tag
    assert np.max(np.abs(got["gn"])) > 0.0, tag
    if mask is not None:
        off = np.asarray(mask) == 0.0
        for k in ("gn", "schur"):
            z = np.concatenate([got[k][off, :].ravel(), got[k][:, off].ravel()])
            assert np.all(z == 0.0) and not np.signbit(z).any(), (tag, k)
        for k in ("jac", "coupling"):
            z = got[k][..., off]
            assert np.all(z == 0.0) and not np.signbit(z).any(), (tag, k)
    return float(np.max(aerr / np.maximum(abar, 1e-300))), float(np.max(serr / np.maximum(sbar, 1e-300)))


@pytest.mark.parametrize("n_steps", [30, 0], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("name", ["cpep-2441", "cpep-2661", "supp-4355", "sym-raw", "sym-log"])
def test_information_matrices(name, n_steps):
    for N in (70, 5):
        d = _case(name, N)
        eng = _engine(d, n_steps)
        w = _weights(d)
        for pw in (0.0, 0.37):
            got = eng.network_information(penalty_weight=pw, want=ALL)
            # (pw = 0: the symbolic model's subject on constant glucose is flat -- test_a_flat_subject_...)
            assert not (got["status"] & jr.FAILED).any() and (pw == 0.0 or not got["status"].any())
            ra, rs = _check_gn_schur((name, N, pw), got, w, pw)
            print(f"{name} S={n_steps} N={N} pw={pw}: A error / bar {ra:.3g}, S error / bar {rs:.3g}")
        alone = eng.network_information(penalty_weight=0.37, want=("gn", "schur"))    # the host never needs the table
        assert alone["jac"] is None and np.array_equal(alone["gn"], got["gn"]) and np.array_equal(alone["schur"], got["schur"])
        if eng.P > 1:
            mask = np.ones(eng.P)
            mask[[0, eng.P // 2, eng.P - 1]] = 0.0
            eng.set_param_mask(mask)
            masked = eng.network_information(penalty_weight=0.37, want=ALL)
            _check_gn_schur((name, N, "mask"), masked, w, 0.37, mask)
            on = mask == 1.0
            assert np.array_equal(masked["jac"][..., on], got["jac"][..., on])
            bad = d["cond"].copy()                # a failed subject's rows: NaN, masked entries still exactly 0
            bad[2] = np.nan
            f = eng.network_information(cond=bad, penalty_weight=0.37, want=ALL)
            assert f["status"][2] == jr.FAILED and np.isnan(f["jac"][2][:, on]).all() and np.all(f["jac"][2][:, ~on] == 0.0)
            assert np.isnan(f["coupling"][2, on]).all() and np.all(f["coupling"][2, ~on] == 0.0)
            _check_gn_schur((name, N, "mask+fail"), f, w, 0.37, mask)
            eng.set_param_mask(None)
        eng.close()


def test_information_matrices_at_the_widest_shapes():
    """the widest tuned shapes, suppression 4-8-8-1 (P = 121) and c-peptide 2-8-8-8-1 (P = 177), and the fallback kernel at
    P = 193 (suppression 4-8-8-8-1); N = 5"""
    from cude.engine import Engine
    N = 5
    s = make_supp_case(N, (4, 3, 5))
    w = jr.out_weights("supp", len(s["tp"]), s["data"])
    for arch, fallback in (((4, (8, 8, 8), "tanh", "softplus"), True), ((4, 8, 2), False)):
        eng = Engine("supp", arch, n_steps=30)
        assert eng.fallback_kernel == fallback and eng.P == (193 if fallback else 121)
        eng.set_population_supp(s["tp"], s["data"])
        nn = ac.biased_params((4, 8, 2), 5) if not fallback else 0.3 * np.random.default_rng(5).standard_normal(193)
        eng.set_params(nn, s["theta"])
        got = eng.network_information(penalty_weight=0.1, want=ALL)
        print(f"P = {eng.P}: A, S error / bar {_check_gn_schur(arch, got, w, 0.1)}")
        eng.close()
    c = make_cpep_case(N, (2, 8, 3))
    eng = Engine("cpep", (2, 8, 3), n_steps=30, n_state=2)
    assert not eng.fallback_kernel and eng.P == 177
    eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
    eng.set_params(c["nn"], c["beta"])
    got = eng.network_information(penalty_weight=0.1, want=ALL)
    print(f"P = 177: A, S error / bar {_check_gn_schur((2, 8, 3), got, np.ones(len(c['tp'])), 0.1)}")
    eng.close()


# ------------------------------------------------------------------------------------- 5. chunking, failure, flat, qform
FOLD = [("cpep-2441", 30), ("cpep-2441", 0), ("supp-4355", 30), ("supp-4355", 0), ("fallback-2441", 30), ("sym-raw", 30)]
EVERYTHING = ALL + ("qform",)


def _cov(P, seed=9):
    m = np.random.default_rng(seed).standard_normal((P, P))
    return m @ m.T / P + 0.1 * np.eye(P)


@pytest.mark.parametrize("name,n_steps", FOLD)
def test_every_chunking_gives_the_same_bits_and_the_restated_fold(name, n_steps):
    N = 70
    d = _case(name, N)
    eng = _engine(d, n_steps)
    cov = _cov(eng.P)
    got = {p: eng.network_information(penalty_weight=0.2, cov=cov, profiled=p, want=EVERYTHING) for p in (False, True)}
    eng.close()
    # the fold restated in numpy on the device's own rows: b, d bit for bit where w_o = 1.  The suppression model's w_o = 1 /
    # scale_s^2 is the library's own rounding of the population's scale, one ulp from numpy's at most: every term then
    # differs by 2^-52 of its size at most, and the sums by that of the terms' magnitudes plus the roundings of the sums
    w = _weights(d)
    want = jr.information(got[True]["jac"], got[True]["jcond"], w, 0.2)
    if d["model"] != "supp":
        assert np.array_equal(got[True]["coupling"], want["coupling"]) and np.array_equal(got[True]["dcond"], want["dcond"])
    else:
        n_out = w.size
        bmag = np.einsum("o,io,iop->ip", w, np.abs(got[True]["jcond"]), np.abs(got[True]["jac"]))
        dmag = np.einsum("o,io,io->i", w, got[True]["jcond"], got[True]["jcond"])
        assert np.all(np.abs(got[True]["coupling"] - want["coupling"]) <= 2.0 ** -52 * (n_out + 2) * bmag)
        assert np.all(np.abs(got[True]["dcond"] - want["dcond"]) <= 2.0 ** -52 * (n_out + 2) * dmag)
    for chunk in (0, 1, 2, 5):
        e2 = _engine(d, n_steps, options=(("profile_chunk", chunk),))
        for p in (False, True):
            other = e2.network_information(penalty_weight=0.2, cov=cov, profiled=p, want=EVERYTHING)
            for k in EVERYTHING:
                assert np.array_equal(other[k], got[p][k], equal_nan=True), (name, chunk, p, k)
        no_q = e2.network_information(penalty_weight=0.2, want=ALL)         # (A summed along the first pass)
        for k in ALL:
            assert np.array_equal(no_q[k], got[True][k], equal_nan=True), (name, chunk, k)
        e2.close()


@pytest.mark.parametrize("name,n_steps", FOLD)
def test_a_nan_conditional_fails_its_subject_alone(name, n_steps):
    N = 70
    d = _case(name, N)
    cond = d["cond"].copy()
    cond[N - 1] = np.nan
    for chunk in (0, 2):
        eng = _engine(d, n_steps, options=(("profile_chunk", chunk),))
        cov = _cov(eng.P)
        full = eng.network_information(penalty_weight=0.2, cov=cov, profiled=True, want=EVERYTHING)
        assert eng.n_failed() == 0
        got = eng.network_information(cond=cond, penalty_weight=0.2, cov=cov, profiled=True, want=EVERYTHING)
        assert eng.n_failed() == 1
        no_q = eng.network_information(cond=cond, penalty_weight=0.2, want=ALL)
        eng.close()
        assert got["status"][N - 1] == jr.FAILED and not got["status"][:N - 1].any()
        for k in ("jac", "jcond", "coupling", "dcond", "qform"):
            assert np.isnan(got[k][N - 1]).all(), (name, k)
            assert np.array_equal(got[k][:N - 1], full[k][:N - 1]), (name, k)      # the others: bit for bit
        for k in ("gn", "schur"):
            assert np.array_equal(no_q[k], got[k]), (name, chunk, k)
        assert np.isfinite(got["gn"]).all() and np.isfinite(got["schur"]).all()
        _check_gn_schur((name, chunk, "fail"), got, _weights(d), 0.2)
        if d["model"] == "supp":
            continue      # (the loss's scale, hence w_o, is a mean over the population: without the subject the weights differ)
        # A and S: the call on the population without that subject, bit for bit
        cut = {k: (v[:N - 1] if k in ("G", "obs", "age", "t2dm") else v) for k, v in d["c"].items()}
        e3 = _engine(dict(d, c=cut, cond=d["cond"][:N - 1]), n_steps, options=(("profile_chunk", chunk),))
        small = e3.network_information(penalty_weight=0.2, want=("gn", "schur"))
        e3.close()
        assert np.array_equal(small["gn"], got["gn"]) and np.array_equal(small["schur"], got["schur"]), (name, chunk)


@pytest.mark.parametrize("space", ["log", "raw"])
def test_a_flat_subject_is_skipped_in_the_schur_term_and_flagged(space):
    """the symbolic model on constant glucose: the production p0 dG / (dG + k) is identically zero, so is its derivative with
    respect to k, d_i = 0 exactly, and with pw = 0 the subject is FLAT"""
    N, flat = 5, 3
    d = _case("sym-" + space, N)
    c = dict(d["c"])
    G = np.array(c["G"], dtype=np.float64)
    G[flat, :] = G[flat, 0]
    d = dict(d, c=dict(c, G=G))
    eng = _engine(d, 30)
    cov = np.array([[0.7]])
    got = eng.network_information(penalty_weight=0.0, cov=cov, profiled=True, want=EVERYTHING)
    assert eng.n_failed() == 0
    assert got["status"][flat] == jr.FLAT and np.count_nonzero(got["status"]) == 1
    assert got["dcond"][flat] == 0.0 and np.all(got["jcond"][flat] == 0.0)
    w = _weights(d)
    _check_gn_schur(("flat", space), got, w, 0.0)
    want = jr.information(got["jac"], got["jcond"], w, 0.0, cov=cov, profiled=True)
    assert np.array_equal(want["status"], got["status"])
    assert np.allclose(got["qform"], want["qform"], rtol=1e-13, atol=0.0)
    assert np.array_equal(got["qform"][flat], 0.7 * got["jac"][flat, :, 0] ** 2)          # z = J for the flat subject
    with_pw = eng.network_information(penalty_weight=0.5, want=("status",))
    assert not with_pw["status"].any()            # d + pw > 0: no longer flat
    eng.close()


@pytest.mark.parametrize("profiled", [False, True])
@pytest.mark.parametrize("name,n_steps", [("cpep-2441", 30), ("supp-4355", 0), ("sym-log", 30)])
def test_quadratic_forms_against_numpy(name, n_steps, profiled):
    N, pw = 70, 0.2
    d = _case(name, N)
    eng = _engine(d, n_steps)
    cov = _cov(eng.P)
    got = eng.network_information(penalty_weight=pw, cov=cov, profiled=profiled, want=EVERYTHING)
    eng.close()
    coef = got["jcond"] / (got["dcond"] + pw)[:, None] if profiled else np.zeros_like(got["jcond"])
    z = got["jac"] - coef[:, :, None] * got["coupling"][:, None, :]               # (numpy rounds the product, then the difference)
    want = np.einsum("ioq,qr,ior->io", z, cov, z)
    bar = 2.0 ** -52 * (2 * eng.P + 8) * np.einsum("ioq,qr,ior->io", np.abs(z), np.abs(cov), np.abs(z))
    err = np.abs(got["qform"] - want)
    live = jr.live_outputs(d["model"], len(d["c"]["tp"]))
    print(f"{name} S={n_steps} profiled={profiled}: qform error / bar {np.max(err / np.maximum(bar, 1e-300)):.3g}")
    assert np.all(err <= bar) and np.all(got["qform"][:, _dead_outputs(d)] == 0.0)
    moving = np.abs(z).max(axis=-1) > 0.0         # (cov is positive definite; the flat subject's rows may be exactly zero)
    assert np.all(got["qform"][moving] > 0.0) and np.count_nonzero(moving[:, live]) >= 0.9 * N * len(live)


def test_argument_and_state_errors():
    from cude._lib import CudeError
    from cude.engine import Engine
    d = _case("cpep-2441", 5)
    eng = _engine(d, 30)
    P = eng.P
    with pytest.raises(CudeError, match="no output requested") as ei:
        eng.network_information(want=())
    assert ei.value.status == -1
    with pytest.raises(CudeError, match="qform_out needs cov") as ei:
        eng.network_information(want=("qform",))
    assert ei.value.status == -1
    for v in (np.nan, np.inf):
        cov = np.eye(P)
        cov[1, 2] = v
        with pytest.raises(CudeError, match="cov must be finite") as ei:
            eng.network_information(cov=cov, want=("qform",))
        assert ei.value.status == -1
    for v in (-1e-300, -1.0, np.nan, np.inf):
        with pytest.raises(CudeError, match="penalty_weight must be finite and >= 0") as ei:
            eng.network_information(penalty_weight=v)
        assert ei.value.status == -1
    with pytest.raises(ValueError):
        eng.network_information(cond=np.zeros(4))
    with pytest.raises(ValueError):
        eng.network_information(cov=np.eye(P + 1), want=("qform",))
    with pytest.raises(ValueError):
        eng.network_information(want=("nonsense",))
    eng.close()
    c = d["c"]
    eng = Engine("cpep", (2, 4, 2), n_steps=30, n_state=2)
    eng.N = 5
    from cude._lib import check
    import ctypes
    n = ctypes.c_int32()
    with pytest.raises(CudeError, match="population not set") as ei:
        check(eng._lib.cude_network_information(eng._h, None, 0.0, None, 0, None, None, None, None,
                                                np.empty(5).ctypes.data, None, None, None))
    state = ei.value.status
    assert state == -3
    with pytest.raises(CudeError, match="population not set"):
        check(eng._lib.cude_n_outputs(eng._h, ctypes.byref(n)))
    eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
    assert eng.n_outputs == len(c["tp"])
    with pytest.raises(CudeError, match="shared parameters not set") as ei:
        eng.network_information()
    assert ei.value.status == state
    eng.set_params(c["nn"], None)
    with pytest.raises(CudeError, match="conditional parameters are not set") as ei:
        eng.network_information()
    assert ei.value.status == state
    got = eng.network_information(cond=d["cond"])  # an explicit vector needs none
    assert np.isfinite(got["gn"]).all()
    eng.close()


# --------------------------------------------------------------------------------------------------------- 6. end to end
def test_expected_information_mirrors():
    """2-4-4-1 (P = 37) at N = 12: the OPG route has rank <= 12, the expected-information route does not"""
    from cude import api
    import scores_ref as sr
    import test_gpu_predictive as tgp
    arch, N = (2, 4, 2), 12
    c = make_cpep_case(N, arch)
    models = tgp._api_models(api, c, arch, N)
    T = len(c["tp"])
    sigma = float(np.sqrt(np.median(sr.cpep_rows_torch(c, arch)[1]) / T))
    pm, sd = -0.6, 0.9
    theta = api.ComponentArray(neural=c["nn"], conditional=c["beta"][:, None])
    try:
        opg = api.network_standard_errors(None, c["nn"], models, c["tp"], c["obs"], sigma, pm, sd, method="grid", n_nodes=9,
                                          n_steps=30)
        exp = api.network_standard_errors(c["beta"], c["nn"], models, c["tp"], c["obs"], sigma, pm, sd, estimator="expected",
                                          n_steps=30)
        info = api.network_information(c["beta"], c["nn"], models, c["tp"], c["obs"], sigma=sigma, prior_omega=sd, n_steps=30)
        cov = api.network_covariance(c["beta"], c["nn"], models, c["tp"], c["obs"], sigma=sigma, prior_omega=sd, n_steps=30)
        se = api.prediction_standard_errors(c["beta"], c["nn"], models, c["tp"], c["obs"], sigma=sigma, prior_omega=sd,
                                            n_steps=30)
        jac, jcond = api.output_jacobian(theta, (models, c["tp"], c["obs"]), n_steps=30)
    finally:
        api.clear_cache()
    P = c["nn"].size
    assert opg.rank <= N < P
    assert exp.rank > N and np.isfinite(exp.se).all() and exp.se.shape == (P,)
    assert exp.n_failed == 0 and info["penalty_weight"] == (sigma / sd) ** 2
    assert np.array_equal(exp.schur, info["schur"]) and np.array_equal(cov, exp.cov)
    assert se.shape == (N, T) and np.all(se >= 0.0) and np.all(se[:, 0] == 0.0) and np.all(se[:, 1:] > 0.0)
    assert jac.shape == (N, T, P) and jcond.shape == (N, T)
    want_j, want_c, _ = jr.cpep_jac_torch(c, arch)
    assert np.all(np.max(np.abs(jac - want_j), axis=-1)[:, 1:] <= _row_bar(want_j[:, 1:], 1e-9))
    # the delta-method variance restated with the joint inverse of the arrowhead matrix, per subject
    pw = info["penalty_weight"]
    Sinv = api._pinv_sym(info["schur"])
    i, o = 4, T - 1
    zt = jac[i, o] - jcond[i, o] / (info["dcond"][i] + pw) * info["coupling"][i]
    own = jcond[i, o] ** 2 / (info["dcond"][i] + pw)
    want = zt @ Sinv @ zt + own
    # (the forward bound of the two nested dot products, for the device's sum and for numpy's)
    bar = 2.0 * 2.0 ** -52 * (2 * P + 8) * (np.abs(zt) @ np.abs(Sinv) @ np.abs(zt) + own)
    assert abs((se[i, o] / sigma) ** 2 - want) <= bar and want > 0.0


def test_suppression_mirrors():
    from cude import api
    N = 5
    s = make_supp_case(N, (4, 3, 5))
    prob = api.SuppressionProblem(api.chain(3, 5, "tanh", input_dims=4))
    p = api.ComponentArray(theta=s["theta"], neural=s["nn"])
    try:
        jac, jcond = api.suppression_output_jacobian(p, (prob, s["data"], s["tp"], 0.0), n_steps=30)
        info = api.suppression_network_information(p, (prob, s["data"], s["tp"], 0.0), n_steps=30)
    finally:
        api.clear_cache()
    T = len(s["tp"])
    assert jac.shape == (N, 3 * T, s["nn"].size) and jcond.shape == (N, 3 * T)
    want_j, want_c, _ = jr.supp_jac_torch(s, (4, 3, 5))
    live = jr.live_outputs("supp", T)
    assert np.all(np.max(np.abs(jac - want_j), axis=-1)[:, live] <= _row_bar(want_j[:, live], 1e-9))
    w = jr.out_weights("supp", T, s["data"])
    A = np.einsum("o,ioq,ior->qr", w, jac, jac)
    assert np.allclose(info["gn"], A, rtol=1e-12, atol=1e-12 * np.max(np.abs(A))) and not info["status"].any()
