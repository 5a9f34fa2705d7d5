"""cude_subject_scores without a GPU: the fold rule restated, Fisher's identity on the oracle alone, and the host-side
pieces of the mirrors (posterior weights, OPG covariance, the loop of train_marginal).

Fisher's identity: with the rule's points and weights held fixed,
    d/d theta sum_i log sum_k exp(a_k + ll_ik + lp_ik) = -1/(2 sigma^2) sum_i sum_k w_ik d SSE_i(x_ik) / d theta,
w_ik the posterior weights of the nodes.  Left: torch autograd through cude_oracle.cpep_loss as one graph; right: built
from per-(subject, node) autograd rows with the fold of scores_ref.  Bar 1e-12 of the largest entry: both sides are the
same few hundred thousand float64 operations in different association orders (measured at N = 5, K = 5: 2.7e-15)."""
import math
import os

import numpy as np
import pytest

import scores_ref as sr
from conftest import make_cpep_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fold_restatement_against_a_scalar_loop():
    """scores_ref.fold (vectorised) against the rule written out per subject and entry in Python floats"""
    rng = np.random.default_rng(5)
    K, N, P = 6, 7, 4
    rows, sse = rng.standard_normal((K, N, P)), rng.random((K, N))
    w = rng.standard_normal((K, N))
    w[2, 3] = 0.0
    rows[2, 3, 1] = np.nan                        # no weight: skipped
    w[4, :] = 0.0
    sse[4, 0] = np.inf
    rows[1, 5, 2] = np.inf                        # weight: subject 5 is bad once
    sse[3, 6] = np.nan                            # ... and subject 6
    s, ws, bad = sr.fold(rows, sse, w)
    for i in range(N):
        acc, a_sse, nb = [0.0] * P, 0.0, 0
        for k in range(K):
            wk = float(w[k, i])
            if wk == 0.0:
                continue
            for q in range(P):
                prod = wk * float(rows[k, i, q])
                acc[q] = acc[q] + prod
            a_sse = a_sse + wk * float(sse[k, i])
            nb += int(not (math.isfinite(sse[k, i]) and all(math.isfinite(v) for v in rows[k, i])))
        assert np.array_equal(s[i], np.array(acc), equal_nan=True) and bad[i] == nb
        assert ws[i] == a_sse or (math.isnan(ws[i]) and math.isnan(a_sse))
    assert list(bad) == [0, 0, 0, 0, 0, 1, 1]
    scores, wsse, failed = sr.finish(s, ws, bad, mask=[1.0, 0.0, 1.0, 1.0])
    assert list(failed) == [False] * 5 + [True, True]
    assert np.all(scores[:, 1] == 0.0) and np.isnan(scores[5:, [0, 2, 3]]).all() and np.isnan(wsse[5:]).all()
    assert np.array_equal(scores[:5, [0, 2, 3]], s[:5][:, [0, 2, 3]])
    # weights None = 1: the plain sum in set order
    s1, _, _ = sr.fold(rows[:2, :5], sse[:2, :5])
    assert np.array_equal(s1, rows[0, :5] + rows[1, :5])


def test_fishers_identity_on_the_oracle():
    from cude import api
    arch, N, K = (2, 4, 2), 4, 3
    c = make_cpep_case(N, arch)
    z, a = api.gauss_hermite_rule(K)
    rng = np.random.default_rng(2)
    center, scale = c["beta"] + 0.1 * rng.standard_normal(N), 0.1 + 0.2 * rng.random(N)
    points = center[None, :] + scale[None, :] * z[:, None]
    base = sr.cpep_rows_torch(c, arch)[1]
    sigma = float(np.sqrt(np.median(base) / len(c["tp"])))
    m = sr.marginal_cpep_torch(c, arch, points, a, sigma, -0.6, 0.9)
    # the reference rows of the GPU tests (one backward pass over per-subject copies of the parameters) are the rows of
    # one backward pass per subject over a shared vector: the same products, summed over fewer zero terms
    for k in range(K):
        fast, sse_k = sr.cpep_rows_torch(c, arch, cond=points[k])
        assert np.array_equal(sse_k, m["sse"][k])
        assert np.max(np.abs(fast - m["rows"][k])) <= 1e-13 * np.max(np.abs(m["rows"][k]))
    assert np.max(np.abs(m["w"].sum(axis=0) - 1.0)) <= 1e-14
    s, _, bad = sr.fold(m["rows"], m["sse"], m["w"])
    assert not bad.any()
    fisher = -s.sum(axis=0) / (2.0 * sigma * sigma)
    err = np.max(np.abs(fisher - m["gradient"])) / np.max(np.abs(m["gradient"]))
    print(f"Fisher's identity, N = {N}, K = {K}: relative error {err:.3g}")
    assert err <= 1e-12
    # the mirror's weight formula on the same terms: logml = logsumexp + log scale
    logml = np.log(np.exp(m["terms"] - m["terms"].max(axis=0)).sum(axis=0)) + m["terms"].max(axis=0) + np.log(scale)
    w = api.posterior_weights(m["terms"], logml, scale)
    assert np.max(np.abs(w - m["w"])) <= 1e-13


def test_posterior_weights_sum_to_one():
    from cude import api
    rng = np.random.default_rng(8)
    K, N = 9, 6
    t = -40.0 + 30.0 * rng.standard_normal((K, N))
    t[3, 1] = -np.inf                             # a bad node
    t[:, 4] = -np.inf                             # a subject without a finite term
    scale = 0.2 + rng.random(N)
    top = np.where(np.isfinite(t).any(axis=0), np.max(t, axis=0), 0.0)
    with np.errstate(divide="ignore"):
        logml = np.log(np.exp(t - top).sum(axis=0)) + top + np.log(scale)
    w = api.posterior_weights(t, logml, scale)
    ok = np.arange(N) != 4
    assert np.max(np.abs(w[:, ok].sum(axis=0) - 1.0)) <= 4 * K * 2.0 ** -52
    assert w[3, 1] == 0.0 and np.all(w[:, 4] == 0.0) and np.all(np.isfinite(w)) and np.all(w >= 0.0)
    # scale None = 1
    assert np.array_equal(api.posterior_weights(t, logml - np.log(scale)), api.posterior_weights(t, logml - np.log(scale), np.ones(N)))


def test_opg_covariance_on_hand_made_numbers():
    from cude import api
    g = np.array([[1.0, 0.0], [0.0, 2.0], [1.0, 2.0]])
    opg = g.T @ g
    assert np.array_equal(opg, [[2.0, 2.0], [2.0, 8.0]])
    cov, se = api.opg_covariance(opg)
    assert np.allclose(cov, [[2.0 / 3.0, -1.0 / 6.0], [-1.0 / 6.0, 1.0 / 6.0]], rtol=1e-14, atol=0)
    assert np.allclose(se, [math.sqrt(2.0 / 3.0), math.sqrt(1.0 / 6.0)], rtol=1e-14)
    # fewer subjects than parameters: rank 1, the pseudo-inverse of v v^T is v v^T / |v|^4
    v = np.array([3.0, 4.0])
    cov, se = api.opg_covariance(np.outer(v, v))
    assert np.allclose(cov, np.outer(v, v) / 625.0, rtol=1e-13, atol=1e-18)
    assert np.allclose(se, [3.0 / 25.0, 4.0 / 25.0], rtol=1e-13)
    # a frozen parameter: zero row and column, zero standard error
    cov, se = api.opg_covariance([[4.0, 0.0], [0.0, 0.0]])
    assert np.array_equal(cov, [[0.25, 0.0], [0.0, 0.0]]) and list(se) == [0.5, 0.0]


def test_train_marginal_loop_on_a_stub_objective():
    """_marginal_em_rounds: L-BFGS per round on (-total, -gradient), the hyperparameters updated between rounds from the
    moments of the round's last accepted point, the trace = total at every round's start and accepted iteration"""
    from cude import api
    calls = []
    A = np.diag([1.0, 10.0, 100.0])

    def objective(x, hyper):
        calls.append((x.copy(), hyper))
        d = x - hyper
        return 0.5 * float(d @ A @ d), A @ d, ("moments", x.copy())

    seen = []

    def update(moments):
        assert moments[0] == "moments"
        seen.append(moments[1])
        return moments[1] + 1.0                   # the next round's optimum: one away from where this one ended

    x0 = np.array([3.0, -2.0, 1.0])
    x, hyper, trace, starts = api._marginal_em_rounds(x0, np.zeros(3), objective, update, rounds=3, iterations=4)
    assert len(seen) == 3 and np.array_equal(hyper, seen[-1] + 1.0) and np.array_equal(x, seen[-1])
    assert starts[0] == 0 and len(starts) == 3 and trace[0] == -0.5 * (9.0 + 40.0 + 100.0)
    first = [x0, seen[0], seen[1]]
    hypers = [np.zeros(3), seen[0] + 1.0, seen[1] + 1.0]
    for r in range(3):
        part = trace[starts[r]:(starts[r + 1] if r < 2 else len(trace))]
        d = first[r] - hypers[r]
        assert part[0] == -0.5 * float(d @ A @ d)                                 # the round's start, at the round's hyper
        assert 1 <= len(part) - 1 <= 4                                            # at most `iterations` accepted iterations
        assert all(b >= a for a, b in zip(part, part[1:])) and part[-1] > part[0]    # total never decreases inside a round
        assert part[-1] == -0.5 * float((seen[r] - hypers[r]) @ A @ (seen[r] - hypers[r]))   # moments = the last accepted point's
    # a non-finite start ends the loop with the trace entry and no update
    x, hyper, trace, starts = api._marginal_em_rounds(np.zeros(2), 1.0, lambda p, h: (np.inf, np.zeros(2), None), update, 2, 3)
    assert trace == [-np.inf] and hyper == 1.0 and len(seen) == 3 and starts == [0]


def test_header_and_mirrors_name_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "cude.h")).read()
    assert "int32_t cude_subject_scores(cude_ctx* ctx, int32_t n_sets, const double* cond_sets, const double* weights," in hdr
    from cude import _lib
    assert "cude_subject_scores" in _lib.exported_symbols()
    jl = open(os.path.join(ROOT, "conditional-ude_amd", "julia", "CUDEHip.jl")).read()
    assert ":cude_subject_scores" in jl
