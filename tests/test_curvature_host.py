"""cude_curvature without a GPU: the reference helper checks itself, so that its own error cannot hide a device error.

tests/curvature_ref.py has two routes to d^2 u / d cond^2: (a) torch double backward through the oracle, exact to rounding;
(b) a stencil over the complex-step first derivatives, thirty times cheaper, which the GPU tests use wherever it is valid.
Here (b) is held to (a) within 1e-10 of the reference array's max-norm -- a tenth of the device's bar GRAD_RTOL = 1e-9 --
for sens2 and for curv, on every non-relu fixed-step case tests/test_gpu_curvature_shapes.py takes route (b) for: the 24
c-peptide shapes (n_state 3, whose first two states are the n_state 2 case: asserted), the 16 suppression shapes, the
general shapes with the three pairs that have no relu.  With relu (b) is wrong by orders of magnitude wherever a
subject's stencil straddles a kink: asserted, so that nobody "simplifies" the GPU test's choice of route (a) there.

The adaptive cases difference the replay of a FIXED step sequence (sensitivity_ref.*_sens_replay), the same arithmetic as a
fixed-step solve with unequal steps; torch cannot walk cude_oracle.replay_steps subject by subject in test time, so the
replay stencil is held to a second stencil of another order and step (4th order, h = 1e-4) on the oracle's own accepted
steps: their truncation errors differ by orders of magnitude, so agreement at 1e-10 bounds both.

Also here: curv = (1/2) d^2 SSE / d cond^2 by differentiating the SSE itself twice; the second-order term dwarfs the
device's bar on the test cases (a kernel that returned info as curv cannot pass); the formulas api.py builds on the
curvature; the C ABI entry."""
import ctypes
import math
import os

import numpy as np
import pytest

import adaptive_cases as ac
import curvature_ref as cr

AGREE = 1e-10                    # a tenth of GRAD_RTOL
GRAD_RTOL = 1e-9                 # tests/test_gpu_sensitivity.py
NO_RELU = [a for a in ac.GENERAL_ACTS if "relu" not in a]
RELU = [a for a in ac.GENERAL_ACTS if "relu" in a]


def _ratio(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _both(model, k, acts=(), stencil=True):
    c, cond, _ = ac.tangent_case(model, k)
    arch = tuple(c["arch"]) + tuple(acts)
    if model == "cpep":
        pop = ac.cpep_population(c)
        a = cr.cpep_curv_torch(c["nn"], c[cond], pop, arch, 30, 3)
        b = cr.cpep_curv(c["nn"], c[cond], pop, arch, 30, 3) if stencil else None
        b2 = cr.cpep_curv(c["nn"], c[cond], pop, arch, 30, 2) if stencil else None
    else:
        a = cr.supp_curv_torch(c["nn"], c[cond], c["data"], c["tp"], arch, 30)
        b = cr.supp_curv(c["nn"], c[cond], c["data"], c["tp"], arch, 30) if stencil else None
        b2 = None
    return a, b, b2


def _agree(tag, model, k, acts=()):
    a, b, b2 = _both(model, k, acts)
    r2, rc = _ratio(b["sens2"], a["sens2"]), _ratio(b["curv"], a["curv"])
    frac = float(np.mean(np.abs(a["curv"] - a["info"]) > 1000 * GRAD_RTOL * np.max(np.abs(a["curv"]))))
    print(f"{tag}: (b) vs (a) sens2 {r2:.2e} curv {rc:.2e}; first order sens {_ratio(b['sens'], a['sens']):.2e} "
          f"score {_ratio(b['score'], a['score']):.2e}; (curv - info) / info {np.min((a['curv'] - a['info']) / a['info']):.1f} "
          f"... {np.max((a['curv'] - a['info']) / a['info']):.1f}; curv < 0 for {np.count_nonzero(a['curv'] < 0)} of "
          f"{a['curv'].size}; |curv - info| > 1000 bars for {frac:.0%}")
    assert r2 <= AGREE and rc <= AGREE
    assert _ratio(b["sens"], a["sens"]) <= 1e-13 and _ratio(b["score"], a["score"]) <= 1e-13
    # curv - info is the second-order sum, from each route's own pieces
    for r in (a, b):
        assert np.max(np.abs((r["curv"] - r["info"]) - r["second"])) <= 1e-12 * np.max(np.abs(r["curv"]))
    assert frac > 0.5                       # a kernel that returned info as curv cannot pass
    if model == "supp":
        assert np.all(a["sens2"][0] == 0.0) and np.all(b["sens2"][0] == 0.0)
    assert np.all(a["sens2"][:, 0] == 0.0) and np.all(b["sens2"][:, 0] == 0.0)
    if b2 is not None:                      # the n_state 2 case is the first two states of the n_state 3 one
        assert _ratio(b2["sens2"], a["sens2"][:2]) <= AGREE and _ratio(b2["curv"], a["curv"]) <= AGREE


@pytest.mark.parametrize("k", range(len(ac.CPEP_SHAPES)), ids=[str(s) for s in ac.CPEP_SHAPES])
def test_stencil_against_double_backward_cpep(k):
    _agree(f"cpep {ac.CPEP_SHAPES[k]}", "cpep", k)


@pytest.mark.parametrize("k", range(len(ac.SUPP_SHAPES)), ids=[str(s) for s in ac.SUPP_SHAPES])
def test_stencil_against_double_backward_supp(k):
    _agree(f"supp {ac.SUPP_SHAPES[k]}", "supp", k)


@pytest.mark.parametrize("acts", NO_RELU, ids=["-".join(a) for a in NO_RELU])
@pytest.mark.parametrize("model,shape", [("cpep", s) for s in ac.CPEP_GENERAL_SHAPES] + [("supp", s) for s in ac.SUPP_GENERAL_SHAPES],
                         ids=str)
def test_stencil_against_double_backward_general_activations(model, shape, acts):
    k = (ac.CPEP_SHAPES if model == "cpep" else ac.SUPP_SHAPES).index(shape)
    _agree(f"{model} {shape} {'-'.join(acts)}", model, k, acts)


@pytest.mark.parametrize("model", ["cpep", "supp"])
def test_the_stencil_is_wrong_across_relu_kinks(model):
    """Where a subject's stencil points straddle a kink of some unit, route (b) differences a function that is not smooth.
    Measured on the general shapes x the two relu pairs: 1.6e-1 ... 2.6e2 of the max-norm (c-peptide), 3.3e1 ... 2.0e3
    (suppression 3x5) -- and 1e-12 on suppression 3x3, whose 12 subjects happen to straddle none: the stencil is not
    wrong everywhere, which is why it cannot be trusted anywhere with relu.  Asserted: the first derivatives agree in every
    case (the kinks hurt the stencil only), and in at least one case per shape list the stencil misses by more than a
    thousand device bars."""
    shapes = ac.CPEP_GENERAL_SHAPES if model == "cpep" else ac.SUPP_GENERAL_SHAPES
    worst = 0.0
    for shape in shapes:
        k = (ac.CPEP_SHAPES if model == "cpep" else ac.SUPP_SHAPES).index(shape)
        for acts in RELU:
            a, b, _ = _both(model, k, acts)
            r2, rc = _ratio(b["sens2"], a["sens2"]), _ratio(b["curv"], a["curv"])
            print(f"{model} {shape} {'-'.join(acts)}: (b) vs (a) sens2 {r2:.2e} curv {rc:.2e}; first order {_ratio(b['sens'], a['sens']):.2e}")
            assert _ratio(b["sens"], a["sens"]) <= 1e-13
            worst = max(worst, min(r2, rc))
    assert worst > 1000 * GRAD_RTOL


# ----------------------------------------------------------------------------- the replay stencil
def _fourth_order(first, cond, h=1e-4):
    return (-first(cond + 2 * h) + 8 * first(cond + h) - 8 * first(cond - h) + first(cond - 2 * h)) / (12 * h)


@pytest.mark.parametrize("model", ["cpep", "supp"])
def test_replay_stencil_against_a_stencil_of_another_order(model):
    import sensitivity_ref as sref
    if model == "cpep":
        arch = ac.CPEP_SHAPES[3]
        c = ac.cpep_case(arch, 3, ac.TP6, ac.cpep_subjects(arch))
        pop = ac.cpep_population(c)
        steps = [ac.cpep_solve(c, pop, i)[1] for i in range(pop.N)]
        ref = cr.cpep_curv_replay(c["nn"], c["beta"], pop, arch, steps)
        other = _fourth_order(lambda x: sref.cpep_sens_replay(c["nn"], x, pop, arch, steps)[0], c["beta"])
    else:
        c, _, _ = ac.tangent_case("supp", 6)
        N = c["theta"].size
        steps = [ac.supp_solve(c, i)[1] for i in range(N)]
        ref = cr.supp_curv_replay(c["nn"], c["theta"], c["data"], c["tp"], c["arch"], steps)
        other = _fourth_order(lambda x: sref.supp_sens_replay(c["nn"], x, c["data"], c["tp"], c["arch"], steps)[0], c["theta"])
    other[:, 0] = 0.0
    r = _ratio(ref["sens2"], other)
    print(f"replay {model}: 6th order h = {cr.STENCIL_H} vs 4th order h = 1e-4: {r:.2e}")
    assert r <= AGREE
    assert np.max(np.abs((ref["curv"] - ref["info"]) - ref["second"])) <= 1e-12 * np.max(np.abs(ref["curv"]))


# ----------------------------------------------------------------------------- curv is half the second derivative of the SSE
@pytest.mark.parametrize("model", ["cpep", "supp"])
def test_curv_is_half_the_second_derivative_of_the_sse(model):
    import torch

    import cude_oracle as o
    c, cond, _ = ac.tangent_case(model, 0 if model == "cpep" else 1)
    x = torch.tensor(c[cond], requires_grad=True)
    if model == "cpep":
        pop = ac.cpep_population(c)
        traj = o.cpep_forward(torch, c["nn"], x, pop, c["arch"], 30, 2)
        obs = torch.tensor(pop.cpeptide)
        sse = sum((traj[ti][0] - obs[:, ti]) ** 2 for ti in range(pop.T))
        a = cr.cpep_curv_torch(c["nn"], c[cond], pop, c["arch"], 30, 2)
    else:
        data = c["data"]
        traj = o.supp_forward(torch, c["nn"], x, data, c["tp"], c["arch"], 30)
        w2 = 1.0 / o.supp_scale(data) ** 2
        sse = sum(float(w2[s]) * (traj[ti][s] - torch.tensor(data[s, ti])) ** 2 for ti in range(len(c["tp"])) for s in range(3))
        a = cr.supp_curv_torch(c["nn"], c[cond], data, c["tp"], c["arch"], 30)
    (g,) = torch.autograd.grad(sse.sum(), x, create_graph=True)
    (g2,) = torch.autograd.grad(g.sum(), x)
    half = 0.5 * g2.numpy()
    print(f"{model}: curv vs (1/2) d2 SSE: {_ratio(a['curv'], half):.2e}; score vs (1/2) d SSE: {_ratio(a['score'], 0.5 * g.detach().numpy()):.2e}")
    assert _ratio(a["curv"], half) <= 1e-12 and _ratio(a["score"], 0.5 * g.detach().numpy()) <= 1e-12
    assert _ratio(a["sse"], sse.detach().numpy()) <= 1e-13


# ----------------------------------------------------------------------------- the formulas api.py builds on the curvature
def test_formulas_against_a_restatement():
    import marginal_ref as mr
    from cude import api
    curv = np.array([4.0, -1.0, 0.0, np.nan, 0.25])
    info = np.array([5.0, 2.0, 1.0, np.nan, 0.5])
    sigma, om, pm = 0.3, 0.6, -1.0
    # observed standard errors: api._standard_errors applied to curv is the restatement
    se = api._standard_errors(curv, np.zeros(5), 6, sigma)
    want = cr.observed_se(curv, sigma)
    assert np.array_equal(se[[0, 4]], [sigma / 2.0, sigma / 0.5]) and se[1] == np.inf and se[2] == np.inf and np.isnan(se[3])
    assert np.array_equal(np.isnan(se), np.isnan(want)) and np.array_equal(se[~np.isnan(se)], want[~np.isnan(want)])
    # map_curvature's classes
    pw = api._penalty_weight(sigma, om)
    assert pw == (sigma / om) ** 2 and api._penalty_weight(sigma, None) == 0.0
    a, b, ratio, cls = cr.map_classes(curv, info, pw)
    assert list(cls) == ["minimum", "not_a_minimum", "minimum", "failed", "minimum"]
    assert list(cr.map_classes(curv, info, 0.0)[3]) == ["minimum", "not_a_minimum", "not_a_minimum", "failed", "minimum"]
    assert np.array_equal(a[[0, 1]], [4.0 + pw, -1.0 + pw]) and ratio[0] == (4.0 + pw) / (5.0 + pw)
    # the Q = 1 rule is the Laplace value f(m) s sqrt(2 pi), in closed form
    z, lw = api.gauss_hermite_rule(1)
    assert z.shape == (1,) and z[0] == 0.0 and abs(lw[0] - 0.5 * math.log(2 * math.pi)) <= 1e-15
    m, sse, T = np.array([-0.7, 0.2]), np.array([0.5, 0.02]), 6
    s = sigma / np.sqrt(np.array([4.0, 0.25]) + pw)
    got = mr.marginal_numpy(z, lw, m[None, :], sse[None, :], m, s, T, sigma, pm, om)["logml"]
    closed = (-(T / 2) * np.log(sigma ** 2) - sse / (2 * sigma ** 2) - 0.5 * ((m - pm) / om) ** 2 - np.log(om)
              - 0.5 * np.log(2 * np.pi) + np.log(s) + 0.5 * np.log(2 * np.pi))
    assert np.max(np.abs(got - closed)) <= 1e-13
    with pytest.raises(ValueError):
        api._information_kind("exact")
    assert api._information_kind("observed") and not api._information_kind("expected")


# ----------------------------------------------------------------------------- the C ABI entry
def test_header_library_and_mirrors_name_the_entry():
    from cude import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "cude.h")).read()
    assert ("int32_t cude_curvature(cude_ctx* ctx, double* sens2, double* curv, double* info, double* score, double* sse);"
            in hdr)
    _lib.load()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "cude_curvature")
    assert "cude_curvature" in _lib.exported_symbols()
    jl = open(os.path.join(root, "conditional-ude_amd", "julia", "CUDEHip.jl")).read()
    for name in (":cude_curvature", "function curvatures(", "function suppression_curvatures(", "function map_curvature(",
                 "information = :expected", "curvature = :expected"):
        assert name in jl, name


def test_null_context_is_an_error_not_an_abort():
    from cude import _lib
    lib = _lib.load()
    assert lib.cude_curvature(None, None, None, None, None, None) == -1      # CUDE_ERR_ARG
    with pytest.raises(_lib.CudeError):
        _lib.check(lib.cude_curvature(None, None, None, None, None, None))
