"""cude_refine_conditional without a GPU: the numpy restatement of its rule (tests/refine_ref.py) against an independent
minimiser, its status codes by construction, how far the result moves under the error the tangent kernels are allowed,
the ABI surface and the cross-compilation of the new translation unit.

The restatement is the yardstick of tests/test_gpu_refine.py; nothing here runs the code under test except the ABI checks.

Cases: the 24-subject 2-4-4-1 c-peptide population and the 16-subject suppression population of tests/conftest.py, fixed
step S = 30, boxes [-4, 3] / [-6, 4], xtol = 1e-7 (the mirrors' default), max_step = 0.5."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import make_cpep_case, make_supp_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPEP_BOX, SUPP_BOX = (-4.0, 3.0), (-6.0, 4.0)


def _case(model):
    import refine_ref as rr
    if model == "cpep":
        c = make_cpep_case(24, (2, 4, 2))
        return c, 24, CPEP_BOX, lambda **kw: rr.cpep_evaluator(c, **kw)
    c = make_supp_case(16)
    return c, 16, SUPP_BOX, lambda **kw: rr.supp_evaluator(c, **kw)


# ----------------------------------------------------------------------------- against an independent minimiser
@pytest.mark.parametrize("model", ["cpep", "supp"])
def test_restatement_finds_the_minimiser_brent_finds_on_the_c_oracle(model):
    """For every subject whose 41-point profile has a unique interior basin (the selection of
    tests/test_gpu_fit.py::test_fit_and_profile_against_the_oracle), scipy's bounded Brent on the C oracle inside the
    scan's bracket and the restatement started from the scan's argmin agree to 2e-6 in x (that test's bar), the
    restatement's objective being no higher; every subject ends converged."""
    import c_oracle as co
    import refine_ref as rr
    from scipy.optimize import minimize_scalar
    c, N, box, make_ev = _case(model)
    if model == "cpep":
        def sse_all(x):
            return co.cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"], (2, 4, 2), c["nn"], x, 30, 2, want_grad=False)["sse"]
    else:
        def sse_all(x):
            return co.supp(c["tp"], c["data"], c["arch"], c["nn"], x, 0.0, 30, want_grad=False)["sse"]
    ev = make_ev()
    values, prof = rr.scan(ev, N, *box)
    x0 = values[np.argmin(prof, axis=0)]
    r = rr.refine(ev, x0, *box)
    print("evals", r["evals"], "status", r["status"])
    assert np.all(r["status"] == rr.CONVERGED)
    assert np.all(r["objective"] <= np.min(prof, axis=0))
    checked = 0
    for i in range(N):
        k = rr.unique_interior_basin(prof, i)
        if k is None:
            continue
        one = lambda v, i=i: sse_all(np.where(np.arange(N) == i, v, 0.0))[i]       # noqa: E731
        b = minimize_scalar(one, bounds=(values[k - 1], values[k + 1]), method="bounded", options=dict(xatol=1e-10))
        print(f"subject {i}: |dx| {abs(r['x'][i] - b.x):.2e}, F - F_brent {r['objective'][i] - b.fun:.2e}")
        assert abs(r["x"][i] - b.x) < 2e-6 and r["objective"][i] <= b.fun * (1 + 1e-10) + 1e-14, (i, r["x"][i], b.x)
        checked += 1
    assert checked >= N // 2


def test_penalised_objective_is_what_is_minimised():
    """With a penalty the half gradient score + pw (x - pc) vanishes at a converged interior result (central difference of
    the restated objective as the independent check)."""
    import refine_ref as rr
    c, N, box, make_ev = _case("cpep")
    ev = make_ev()
    pw, pc = 0.35, -0.6
    r = rr.refine(ev, np.zeros(N), *box, pw=pw, pc=pc)
    assert np.all(r["status"] == rr.CONVERGED)
    F = lambda x: ev(x)[2] + pw * (x - pc) ** 2                                     # noqa: E731
    assert np.allclose(F(r["x"]), r["objective"], rtol=1e-13)
    d = 1e-4
    assert np.all(F(r["x"] + d) >= r["objective"] - 1e-10) and np.all(F(r["x"] - d) >= r["objective"] - 1e-10)


# ----------------------------------------------------------------------------- status codes by construction
def test_constant_glucose_ends_flat():
    import refine_ref as rr
    c = make_cpep_case(24, (2, 4, 2))
    c["G"] = c["G"].copy()
    c["G"][5, :] = c["G"][5, 0]                              # glucose never rises: no production, info = score = 0
    r = rr.refine(rr.cpep_evaluator(c), np.zeros(24), *CPEP_BOX)
    assert r["status"][5] == rr.FLAT and r["evals"][5] == 1 and r["x"][5] == 0.0 and r["info"][5] == 0.0
    assert np.all(np.delete(r["status"], 5) == rr.CONVERGED)


def test_box_that_excludes_the_basin_ends_at_bound():
    import refine_ref as rr
    c, N, box, make_ev = _case("cpep")
    ev = make_ev()
    values, prof = rr.scan(ev, N, *box)
    i = next(i for i in range(N) if rr.unique_interior_basin(prof, i) is not None)
    xs = rr.refine(ev, values[np.argmin(prof, axis=0)], *box)["x"][i]
    lo, hi = xs + 0.2, xs + 0.7                              # the basin lies below the box: downhill ends at `lo`
    r = rr.refine(ev, np.full(N, hi), lo, hi)
    assert r["status"][i] == rr.AT_BOUND and r["x"][i] == lo
    assert np.all((r["x"] >= lo) & (r["x"] <= hi))


def test_two_evaluations_end_max_evals():
    import refine_ref as rr
    c, N, box, make_ev = _case("supp")
    r = rr.refine(make_ev(), np.zeros(N), *box, max_evals=2)
    assert np.all(r["status"] == rr.MAX_EVALS) and np.all(r["evals"] == 2)
    r1 = rr.refine(make_ev(), np.zeros(N), *box, max_evals=1)
    assert np.all(r1["status"] == rr.MAX_EVALS) and np.all(r1["evals"] == 1) and np.all(r1["x"] == 0.0)


def test_nan_glucose_fails_one_subject_and_leaves_the_others():
    import refine_ref as rr
    c = make_cpep_case(24, (2, 4, 2))
    clean = rr.refine(rr.cpep_evaluator(c), np.full(24, 5.0), *CPEP_BOX)
    c["G"] = c["G"].copy()
    c["G"][9, 2] = np.nan
    r = rr.refine(rr.cpep_evaluator(c), np.full(24, 5.0), *CPEP_BOX)
    assert r["status"][9] == rr.FAILED and r["x"][9] == 3.0 and np.isposinf(r["objective"][9]) and r["evals"][9] == 1
    ok = np.arange(24) != 9
    for k in ("x", "objective", "sse", "info", "evals", "status"):
        assert np.array_equal(r[k][ok], clean[k][ok]), k


# ----------------------------------------------------------------------------- the kernels' accepted error
def test_result_under_the_tangent_kernels_accepted_error():
    """cude_sensitivity's score and info are held to 1e-9 of the oracle's.  The restatement re-run with every score and
    info multiplied by 1 +- 1e-9, together and in opposite directions, from the scan's argmin and from 0, both cases, at
    the mirrors' default xtol = 1e-7:

      (a) max |dx| / (1 + |x|) over all runs          1.8e-14 (far below xtol: the last, superlinear step lands within
                                                               rounding of the minimiser whichever run takes it)
      (b) largest share of subjects whose `evals`     0 of 24 (c-peptide), 0 of 16 (suppression)
          changes

    measured here on the reference restatement (printed below); no status changes and no `evals` changes by more than
    one.  tests/test_gpu_refine.py takes its bars from these two numbers: 10 x max((a), xtol) in x, and `evals` equal
    except for at most 2 x (b) of the subjects, there by one.

    Why the default is not 1e-9: at xtol = 1e-9 the same study gives (a) = 1.0e-9 and (b) = 3 of 24 / 1 of 16, but the
    counts that change do so by up to FIVE evaluations (12 -> 7, 8 -> 11), so "by one at the most" does not hold for the
    restatement itself; with the SSE disturbed at the level of its own rounding (3e-14 relative) 10 of the 16
    suppression subjects change, by up to 13.  Step 5 accepts on a comparison of two objective values; steps shorter
    than the width over which the SSE is flat to rounding (~1e-7 in x) are accepted or rejected by noise, and an
    iteration asked to go on until its steps are 1e-9 wanders there.  At 1e-8: (b) = 1 of 24, by one; under SSE noise up
    to 11.  At 1e-7 nothing changes under the study above.  Larger values stop too early for the 1e-10 relative bar on the
    objective (3e-7: 7.5e-10 above Brent's for the subject with the smallest SSE, 8e-5; 1e-6: 1.3e-10 for another)."""
    import refine_ref as rr
    import inspect
    xtol = inspect.signature(rr.refine).parameters["xtol"].default
    assert xtol == 1e-7
    worst_dx, worst_share = 0.0, {}
    for model in ("cpep", "supp"):
        c, N, box, make_ev = _case(model)
        values, prof = rr.scan(make_ev(), N, *box)
        for name, x0 in (("scan", values[np.argmin(prof, axis=0)]), ("zero", np.zeros(N))):
            base = rr.refine(make_ev(), x0, *box)
            assert np.all(base["status"] == rr.CONVERGED)
            for f in (1 + 1e-9, 1 - 1e-9):
                for tag, kw in (("same", dict(f_info=f, f_score=f)), ("opposite", dict(f_info=f, f_score=1.0 / f))):
                    r = rr.refine(make_ev(**kw), x0, *box)
                    dx = float(np.max(np.abs(r["x"] - base["x"]) / (1 + np.abs(base["x"]))))
                    changed = int(np.sum(r["evals"] != base["evals"]))
                    print(f"{model} {name} {f - 1:+.0e} {tag}: max|dx|/(1+|x|) {dx:.2e}, evals changed {changed} of {N}")
                    assert np.array_equal(r["status"], base["status"])
                    assert np.max(np.abs(r["evals"] - base["evals"])) <= 1
                    worst_dx = max(worst_dx, dx)
                    worst_share[model] = max(worst_share.get(model, 0), changed)
    print(f"(a) = {worst_dx:.2e}; (b) = {worst_share}")
    # the recorded numbers still describe the restatement (so that the GPU bars derived from them stay justified)
    assert worst_dx <= 1e-11
    assert worst_share["cpep"] == 0 and worst_share["supp"] == 0


# ----------------------------------------------------------------------------- ABI
PROTO = ("int32_t cude_refine_conditional(cude_ctx* ctx, const double* x0, double lower, double upper, int32_t max_evals,")


def test_symbol_is_declared_and_exported():
    from cude import _lib, engine
    hdr = open(os.path.join(ROOT, "include", "cude.h")).read()
    assert PROTO in hdr
    for k, name in enumerate(("CONVERGED", "AT_BOUND", "MAX_EVALS", "FLAT", "FAILED")):
        assert f"#define CUDE_REFINE_{name} {k}" in hdr and getattr(engine, f"REFINE_{name}") == k
    for cite in ("src/parameter-estimation.jl:272-307", "suppression_model.jl:179-222", "c-peptide/03-symreg.jl:94-106",
                 "src/saem.jl:74-84", '"refine_fused"', "CUDE_REFINE_FUSED"):
        assert cite in hdr, cite
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "cude_refine_conditional")
    assert "cude_refine_conditional" in _lib.exported_symbols()


def test_null_context_returns_a_status():
    from cude import _lib
    lib = _lib.load()
    out = np.zeros(4)
    args = (None, None, -4.0, 3.0, 40, 1e-7, 0.5, 0.0, 0.0, out.ctypes.data_as(ctypes.c_void_p), None, None, None, None, None)
    assert lib.cude_refine_conditional(*args) == -1                           # CUDE_ERR_ARG, no abort
    assert b"null context" in lib.cude_last_error()
    with pytest.raises(_lib.CudeError):
        _lib.check(lib.cude_refine_conditional(*args))


def test_restatement_and_header_state_the_same_constants():
    """One rule, stated in the header, the kernel source and the restatement: the constants agree."""
    import inspect
    import refine_ref as rr
    hdr = open(os.path.join(ROOT, "include", "cude.h")).read()
    src = open(os.path.join(ROOT, "conditional-ude_amd", "csrc", "cude_refine.hip")).read()
    ref = inspect.getsource(rr.refine)
    assert "lambda = 1e-3" in hdr and "kRefLambda0 = 1e-3" in src and "np.full(N, 1e-3)" in ref
    assert "max(lambda / 10, 1e-12)" in hdr and "kRefLambdaMin = 1e-12" in src and "np.maximum(lam / 10.0, 1e-12)" in ref
    assert "lambda <- 10 lambda" in hdr and "s.lam * 10.0" in src and "lam * 10.0" in ref
    sig = inspect.signature(rr.refine).parameters
    from cude.engine import Engine
    eng = inspect.signature(Engine.refine_conditional).parameters
    for k in ("max_evals", "xtol", "max_step"):
        assert sig[k].default == eng[k].default
    assert (eng["max_evals"].default, eng["xtol"].default, eng["max_step"].default) == (40, 1e-7, 0.5)


def test_search_method_does_not_touch_the_new_entry_point(monkeypatch):
    """api.estimate_conditional(method="search") -- the default -- is today's call of fit_conditional and nothing else;
    method="newton" is one profile launch and one refinement."""
    from cude import api
    calls = []

    class FakeEngine:
        N = 3

        def set_params(self, nn, cond):
            calls.append(("set_params",))

        def fit_conditional(self, lo, hi, n_grid=41, n_iters=48, penalty_weight=0.0, penalty_center=0.0):
            calls.append(("fit", lo, hi, n_grid, n_iters, penalty_weight, penalty_center))
            return np.zeros(3), np.ones(3), np.ones(3)

        def profile_conditional(self, values):
            calls.append(("profile", len(values)))
            return (np.asarray(values)[:, None] - np.array([-1.0, 0.0, 0.5])) ** 2

        def refine_conditional(self, x0=None, lower=-4.0, upper=3.0, **kw):
            calls.append(("refine", np.array(x0, dtype=float), lower, upper, kw))
            return dict(x=np.array(x0, dtype=float), objective=np.zeros(3), sse=np.zeros(3), info=np.full(3, 2.0),
                        evals=np.ones(3, np.int32), status=np.zeros(3, np.int32))

    class FakePop:
        engine = FakeEngine()
    monkeypatch.setattr(api, "_population", lambda *a, **k: FakePop())
    x, sse = api.estimate_conditional(["m"] * 3, [0.0, 1.0], None, [0.1])
    assert [c[0] for c in calls] == ["set_params", "fit"] and calls[1][1:] == (-4.0, 1.0, 41, 48, 0.0, 0.0)
    del calls[:]
    x, sse, info = api.estimate_conditional(["m"] * 3, [0.0, 1.0], None, [0.1], method="newton", return_info=True)
    assert [c[0] for c in calls] == ["set_params", "profile", "refine"] and calls[1][1] == 41
    assert np.allclose(calls[2][1], [-1.0, 0.0, 0.5]) and np.all(info == 2.0)        # each subject's grid argmin
    del calls[:]
    api.estimate_conditional(["m"] * 3, [0.0, 1.0], None, [0.1], method="newton", n_grid=0, initial_beta=-2.0)
    assert [c[0] for c in calls] == ["set_params", "refine"] and np.all(calls[1][1] == -2.0)
    with pytest.raises(ValueError):
        api.estimate_conditional(["m"] * 3, [0.0, 1.0], None, [0.1], method="lbfgs")
    # the fit's info stands in for the second solve of the standard errors
    monkeypatch.setattr(api, "sensitivities", lambda *a, **k: pytest.fail("a second solve"))
    se = api.conditional_standard_errors(np.zeros(3), [0.1], ["m"] * 3, [0.0, 1.0, 2.0, 3.0], None, info=np.full(3, 4.0),
                                         sse=np.full(3, 8.0))
    assert np.all(se == np.sqrt(8.0 / 4) / 2.0)


# ----------------------------------------------------------------------------- the new translation unit
def test_cude_refine_cross_compiles_for_gfx950(tmp_path):
    csrc = os.path.join(ROOT, "conditional-ude_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail(f"{hipcc} not found: the library cannot be built here either")
    procs = [subprocess.Popen([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only",
                               f"-DCUDE_REFINE_PART={k}", "-c", os.path.join(csrc, "cude_refine.hip"), "-o",
                               str(tmp_path / f"refine_p{k}.o")], stderr=subprocess.PIPE) for k in range(4)]
    for k, p in enumerate(procs):
        _, err = p.communicate()
        assert p.returncode == 0, f"part {k}: {err.decode()[-2000:]}"
        assert os.path.getsize(tmp_path / f"refine_p{k}.o") > 10000
