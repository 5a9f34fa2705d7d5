"""cude_network_information without a GPU: the algebra its outputs stand for, restated in numpy (jacobian_ref.information);
the api functions built on it, on a stub engine; the signature in the header, the ctypes table and the Julia module; and
the oracle-only identity that ties the Jacobian rows to the score rows of tests/scores_ref.py."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import jacobian_ref as jr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, N_OUT, P = 4, 3, 5


def _random_tables(seed=1):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, N_OUT, P)), rng.standard_normal((N, N_OUT)), 0.5 + rng.random(N_OUT)


def _arrowhead(J, jc, w, pw):
    """[[A, B], [B^T, D + pw I]] of the joint least-squares problem in (theta, cond_1 ... cond_N)"""
    A = np.einsum("o,ioq,ior->qr", w, J, J)
    B = np.einsum("o,io,ioq->qi", w, jc, J)
    D = np.diag(np.einsum("o,io,io->i", w, jc, jc) + pw)
    return np.block([[A, B], [B.T, D]])


@pytest.mark.parametrize("pw", [0.0, 0.3])
def test_schur_complement_is_the_joint_inverse_block(pw):
    J, jc, w = _random_tables()
    r = jr.information(J, jc, w, pw)
    assert not r["status"].any()
    full = np.linalg.inv(_arrowhead(J, jc, w, pw))
    assert np.allclose(full[:P, :P], np.linalg.inv(r["schur"]), rtol=1e-10, atol=1e-12)
    assert np.allclose(r["gn"], _arrowhead(J, jc, w, pw)[:P, :P], rtol=1e-14)
    assert np.allclose(r["coupling"], _arrowhead(J, jc, w, pw)[:P, P:].T, rtol=1e-13)
    assert np.allclose(r["schur"], r["schur"].T, rtol=0, atol=1e-14)


@pytest.mark.parametrize("pw", [0.0, 0.3])
def test_delta_method_variance_is_the_full_quadratic_form(pw):
    J, jc, w = _random_tables(2)
    r0 = jr.information(J, jc, w, pw)
    r = jr.information(J, jc, w, pw, cov=np.linalg.inv(r0["schur"]), profiled=True)
    full = np.linalg.inv(_arrowhead(J, jc, w, pw))
    den = r["dcond"] + pw
    for i in range(N):
        for o in range(N_OUT):
            g = np.zeros(P + N)                   # gradient of yhat_io in the joint parameters
            g[:P], g[P + i] = J[i, o], jc[i, o]
            assert np.isclose(r["qform"][i, o] + jc[i, o] ** 2 / den[i], g @ full @ g, rtol=1e-9, atol=1e-12)
    # not profiled: z = J
    plain = jr.information(J, jc, w, pw, cov=np.eye(P))
    assert np.allclose(plain["qform"], np.einsum("iop,iop->io", J, J), rtol=1e-14)


def test_flat_and_failed_subjects():
    J, jc, w = _random_tables(3)
    jc[1, :] = 0.0                                # flat at pw = 0
    J[2, 1, 3] = np.nan                           # failed
    r = jr.information(J, jc, w, 0.0, cov=np.eye(P), profiled=True)
    assert list(r["status"]) == [0, jr.FLAT, jr.FAILED, 0]
    assert np.isnan(r["jac"][2]).all() and np.isnan(r["jcond"][2]).all() and np.isnan(r["coupling"][2]).all()
    assert np.isnan(r["dcond"][2]) and np.isnan(r["qform"][2]).all()
    keep = [0, 3]
    clean = jr.information(J[keep], jc[keep], w, 0.0, cov=np.eye(P), profiled=True)
    flat_only = np.einsum("o,oq,or->qr", w, J[1], J[1])
    assert np.allclose(r["gn"], clean["gn"] + flat_only, rtol=1e-13)                 # the flat subject counts in A ...
    assert np.allclose(r["schur"], clean["schur"] + flat_only, rtol=1e-12, atol=1e-13)     # ... and has no Schur term
    assert np.allclose(r["qform"][1], np.einsum("op,op->o", J[1], J[1]), rtol=1e-14)   # z = J
    assert np.array_equal(r["qform"][keep], clean["qform"]) and np.array_equal(r["coupling"][keep], clean["coupling"])
    assert np.all(r["coupling"][1] == 0.0) and r["dcond"][1] == 0.0
    # with a penalty the same subject is no longer flat
    assert list(jr.information(J, jc, w, 0.1)["status"]) == [0, 0, jr.FAILED, 0]
    # a failure the rows do not show (the solve's SSE)
    assert list(jr.information(J[keep], jc[keep], w, 0.0, bad=[False, True])["status"]) == [0, jr.FAILED]


def test_masked_entries_are_exactly_zero():
    J, jc, w = _random_tables(4)
    J[3, 0, 1] = np.inf                           # a failed subject: NaN row, masked entries still 0
    mask = np.array([1.0, 0.0, 1.0, 1.0, 0.0])
    r = jr.information(J, jc, w, 0.2, mask=mask, cov=np.eye(P), profiled=True)
    off = mask == 0.0
    for k in ("jac", "coupling"):
        z = r[k][..., off]
        assert np.all(z == 0.0) and not np.signbit(z).any(), k
    for k in ("gn", "schur"):
        assert np.all(r[k][off, :] == 0.0) and np.all(r[k][:, off] == 0.0), k
    assert np.isnan(r["jac"][3][:, ~off]).all() and r["status"][3] == jr.FAILED
    free = jr.information(J[:3][..., ~off], jc[:3], w, 0.2)
    assert np.allclose(r["schur"][np.ix_(~off, ~off)], free["schur"], rtol=1e-13)


# ----------------------------------------------------------------------------------------------- the api on a stub engine
class _StubEngine:
    def __init__(self, J, jc, w):
        self.J, self.jc, self.w = J, jc, w
        self.N, self.P = J.shape[0], J.shape[2]
        self.calls = []

    def set_params(self, nn, cond):
        self.params = (np.asarray(nn), None if cond is None else np.asarray(cond))

    def network_information(self, cond=None, penalty_weight=0.0, cov=None, profiled=False, want=()):
        self.calls.append(dict(penalty_weight=penalty_weight, cov=cov, profiled=profiled, want=tuple(want)))
        r = jr.information(self.J, self.jc, self.w, penalty_weight, cov=cov, profiled=profiled)
        return {k: (r[k] if k in want else None) for k in ("jac", "jcond", "gn", "coupling", "dcond", "schur", "qform", "status")}

    def n_failed(self):
        return 0


@pytest.fixture
def stub(monkeypatch):
    from cude import api
    J, jc, w = _random_tables(5)
    J[:, 0], jc[:, 0] = 0.0, 0.0                  # the column of t_0
    eng = _StubEngine(J, jc, np.ones(N_OUT))
    pop = SimpleNamespace(engine=eng, N=N, T=N_OUT, shared=None)
    monkeypatch.setattr(api, "_population", lambda *a, **k: pop)
    monkeypatch.setattr(api, "_supp_population", lambda *a, **k: pop)
    return api, eng, ([object()] * N, np.arange(N_OUT, dtype=float), np.zeros((N, N_OUT)))


def test_api_information_covariance_and_prediction_errors(stub):
    api, eng, (models, tp, data) = stub
    betas, nn, sigma, omega = np.zeros(N), np.zeros(P), 0.7, 1.4
    pw = (sigma / omega) ** 2
    info = api.network_information(betas, nn, models, tp, data, sigma=sigma, prior_omega=omega)
    want = jr.information(eng.J, eng.jc, eng.w, pw)
    assert info["penalty_weight"] == pw and eng.calls[-1]["penalty_weight"] == pw
    for k in ("gn", "schur", "coupling", "dcond", "status"):
        assert np.array_equal(info[k], want[k]), k
    assert api.network_information(betas, nn, models, tp, data, sigma=sigma)["penalty_weight"] == 0.0
    cov = api.network_covariance(betas, nn, models, tp, data, sigma=sigma, prior_omega=omega)
    assert np.allclose(cov, sigma ** 2 * np.linalg.inv(want["schur"]), rtol=1e-10)
    se = api.prediction_standard_errors(betas, nn, models, tp, data, sigma=sigma, prior_omega=omega)
    assert eng.calls[-1]["profiled"] and eng.calls[-1]["cov"] is not None and "qform" in eng.calls[-1]["want"]
    full = np.linalg.inv(_arrowhead(eng.J, eng.jc, eng.w, pw))
    for i in range(N):
        for o in range(N_OUT):
            g = np.zeros(P + N)
            g[:P], g[P + i] = eng.J[i, o], eng.jc[i, o]
            assert np.isclose(se[i, o], sigma * np.sqrt(g @ full @ g), rtol=1e-9, atol=1e-14)
    assert np.all(se[:, 0] == 0.0) and np.all(se >= 0.0)
    jac, jcond = api.output_jacobian(api.ComponentArray(neural=nn, conditional=betas), (models, tp, data))
    assert np.array_equal(jac, eng.J) and np.array_equal(jcond, eng.jc)
    p = api.ComponentArray(theta=betas, neural=nn)
    jac, jcond = api.suppression_output_jacobian(p, (None, data, tp, 0.0))
    assert np.array_equal(jac, eng.J)
    sinfo = api.suppression_network_information(p, (None, data, tp, 0.0), sigma=sigma, prior_omega=omega)
    assert np.array_equal(sinfo["schur"], want["schur"])


def test_network_standard_errors_estimators(stub, monkeypatch):
    api, eng, (models, tp, data) = stub
    rng = np.random.default_rng(6)
    g = rng.standard_normal((3, P))
    ms = SimpleNamespace(opg=g.T @ g, gradient=g.sum(axis=0), total=-12.5)
    seen = {}

    def fake_marginal_score(*args, **kwargs):
        seen["args"], seen["kwargs"] = args, kwargs
        return ms
    monkeypatch.setattr(api, "marginal_score", fake_marginal_score)
    betas, nn = np.zeros(N), np.zeros(P)
    # "opg", the default: what the function returned before it had the keyword
    cov, se = api.opg_covariance(ms.opg)
    for kw in ({}, {"estimator": "opg"}):
        r = api.network_standard_errors(betas, nn, models, tp, data, 0.7, -0.6, 1.4, method="grid", n_nodes=9, **kw)
        assert seen["kwargs"] == {"method": "grid", "n_nodes": 9} and len(seen["args"]) == 8
        assert np.array_equal(r.cov, cov) and np.array_equal(r.se, se) and np.array_equal(r.opg, ms.opg)
        assert r.rank == 3 and np.array_equal(r.gradient, ms.gradient) and r.total == -12.5
        assert sorted(vars(r)) == ["cov", "gradient", "opg", "rank", "se", "total"]
    seen.clear()
    r = api.network_standard_errors(betas, nn, models, tp, data, 0.7, -0.6, 1.4, estimator="expected")
    assert not seen                               # no marginal scores on this route
    want = jr.information(eng.J, eng.jc, eng.w, (0.7 / 1.4) ** 2)
    assert np.array_equal(r.schur, want["schur"]) and r.rank == P
    assert np.allclose(r.cov, 0.49 * np.linalg.inv(want["schur"]), rtol=1e-10)
    assert np.allclose(r.se, np.sqrt(np.diag(r.cov)), rtol=1e-14)
    with pytest.raises(ValueError):
        api.network_standard_errors(betas, nn, models, tp, data, 0.7, -0.6, 1.4, estimator="observed")
    with pytest.raises(TypeError):
        api.network_standard_errors(betas, nn, models, tp, data, 0.7, -0.6, 1.4, estimator="expected", n_nodes=9)


# ------------------------------------------------------------------------------------------------------- the signature
KINDS = ["ptr", "ptr", "f64", "ptr", "i32"] + ["ptr"] * 8


def test_header_ctypes_and_julia_declare_the_same_signature():
    import ctypes as C
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "cude.h")).read(), flags=re.S)
    m = re.search(r"int32_t\s+cude_network_information\s*\(([^;]*?)\)\s*;", hdr)
    params = [p.strip() for p in m.group(1).split(",")]
    assert [("ptr" if "*" in p else "f64" if p.startswith("double") else "i32") for p in params] == KINDS
    assert [p.split()[-1].lstrip("*") for p in params] == ["ctx", "cond", "penalty_weight", "cov", "profiled", "jac_out", "jcond_out",
                                                          "gn_out", "coupling_out", "dcond_out", "schur_out", "qform_out",
                                                          "status_out"]
    assert params[-1].startswith("int32_t*") and re.search(r"int32_t\s+cude_n_outputs\s*\(cude_ctx\*\s*ctx,\s*int32_t\*\s*n_out\)", hdr)
    from cude import _lib
    ret, args = _lib._SIGNATURES["cude_network_information"]
    assert ret is C.c_int32
    assert [{C.c_void_p: "ptr", C.c_double: "f64", C.c_int32: "i32"}[a] for a in args] == KINDS
    assert {"cude_network_information", "cude_n_outputs"} <= set(_lib.exported_symbols())
    jl = open(os.path.join(ROOT, "conditional-ude_amd", "julia", "CUDEHip.jl")).read()
    call = jl[jl.index("(:cude_network_information, LIB)"):]
    types = re.search(r"Int32,\s*\((.*?)\),\s*c\.h", call, flags=re.S).group(1)
    kinds = [("ptr" if t.strip().startswith("Ptr") else "f64" if t.strip() == "Float64" else "i32") for t in types.split(",")]
    assert kinds == KINDS
    assert ":cude_n_outputs" in jl and "network_information, n_outputs" in jl


# ----------------------------------------------------------------------------------------------- the oracle-only identity
def test_jacobian_contracted_with_the_residuals_is_the_score_row():
    """N = 4, 2-4-4-1, 30 steps: sum_o 2 w_o r_io J_io of the torch-autograd Jacobian of cude_oracle.cpep_forward equals the
    autograd rows of the per-subject SSE (scores_ref.cpep_rows_torch): two backward passes over the same graph"""
    import scores_ref as sr
    from conftest import make_cpep_case
    arch = (2, 4, 2)
    c = make_cpep_case(4, arch)
    jac, jcond, y = jr.cpep_jac_torch(c, arch)
    rows, sse = sr.cpep_rows_torch(c, arch)
    r = y - c["obs"]
    assert np.allclose((r * r).sum(axis=1), sse, rtol=1e-13)
    mine = 2.0 * np.einsum("io,iop->ip", r, jac)
    err = np.max(np.abs(mine - rows), axis=1) / np.max(np.abs(rows), axis=1)
    print(f"Jacobian against score rows: relative error {np.max(err):.3g}")
    assert np.all(err <= 1e-12)
    assert np.all(jac[:, 0] == 0.0) and np.all(jcond[:, 0] == 0.0) and np.all(np.abs(jac[:, 1:]).max(axis=-1) > 0.0)
    # the same for the suppression model, with the loss's weights
    from conftest import make_supp_case
    s = make_supp_case(4, (4, 3, 5))
    jac, jcond, y = jr.supp_jac_torch(s, (4, 3, 5))
    rows, sse = sr.supp_rows_torch(s, (4, 3, 5))
    T = len(s["tp"])
    r = y - s["data"].transpose(2, 1, 0).reshape(4, 3 * T)
    mine = 2.0 * np.einsum("o,io,iop->ip", jr.out_weights("supp", T, s["data"]), r, jac)
    assert np.all(np.max(np.abs(mine - rows), axis=1) <= 1e-12 * np.max(np.abs(rows), axis=1))
    assert np.all(jac[:, 0::3] == 0.0) and np.all(jac[:, :3] == 0.0)
