"""The Levenberg-Marquardt rule of cude_train_lm as restated in tests/lm_ref.py, on a small synthetic arrowhead least-squares
problem (no GPU): yhat_io = exp(c_i) sum_q theta_q phi_q(o), one shared block theta (P = 3) and one scalar per subject."""
import os
import re

import numpy as np

import lm_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, N, T = 3, 7, 6
PHI = np.cos(np.outer(np.arange(P) + 1.0, np.linspace(0.1, 1.3, T)))       # (P, T)
THETA_TRUE = np.array([1.0, -0.4, 0.7])
C_TRUE = np.linspace(-0.3, 0.4, N)


def _model(theta, c):
    return np.exp(c)[:, None] * (theta @ PHI)[None, :]                      # (N, T)


Y = _model(THETA_TRUE, C_TRUE)


def _jac(theta, c):
    J = np.exp(c)[:, None, None] * PHI.T[None, :, :]                        # (N, T, P)
    return J, _model(theta, c)                                              # jc = yhat itself


def _info(theta, c):
    J, jc = _jac(theta, c)
    return np.einsum("iop,ioq->pq", J, J), np.einsum("io,iop->pi", jc, J), np.sum(jc * jc, axis=1)


def _loss(theta, c):
    return float(np.sum((_model(theta, c) - Y) ** 2) / N)


def _grad(theta, c):
    J, jc = _jac(theta, c)
    r = _model(theta, c) - Y
    return _loss(theta, c), 2.0 / N * np.einsum("io,iop->p", r, J), 2.0 / N * np.sum(r * jc, axis=1)


def _losses(thetas, cs):
    return np.array([_loss(t, c) for t, c in zip(thetas, cs)])


def _start():
    rng = np.random.default_rng(4)
    return THETA_TRUE * (1.0 + 0.05 * rng.standard_normal(P)), C_TRUE + 0.05 * rng.standard_normal(N)


def test_elimination_equals_the_dense_solve_and_pred_is_positive():
    theta, c = _start()
    A, B, d = _info(theta, c)
    _, g_t, g_c = _grad(theta, c)
    ghat = 0.5 * N * np.concatenate([g_t, g_c])
    H, M = lr.dense_system(A, B, d)
    for mu in (1e-6, 1e-2, 1e2):
        dense = lr.dense_step(H, M, ghat, mu)
        elim = lr.eliminated_step(A, B, d, ghat, mu)
        assert np.max(np.abs(dense - elim)) <= 1e-9 * np.max(np.abs(dense))
        assert lr.backward_error(H, M, ghat, mu, elim) <= 64 * lr.eta_bar(N, P)
        assert np.sum(lr.pred_terms(ghat, M, dense, mu)) > 0.0
    # the linear model of F = N loss predicts the decrease of a small step: F(x) - F(x + delta) ~ 2 pred - delta^T (H + 2 mu M) delta
    delta = lr.dense_step(H, M, ghat, 1e2)
    pred = np.sum(lr.pred_terms(ghat, M, delta, 1e2))
    actual = N * (_loss(theta, c) - _loss(theta + delta[:P], c + delta[P:]))
    assert 0.0 < actual and abs(actual - (2.0 * pred - delta @ (H + 2e2 * np.diag(M)) @ delta)) <= 0.05 * actual


def test_scaling_floor_and_flat_subject():
    A = np.diag([4.0, 0.0, 1e-12])
    d = np.array([2.0, 0.0])
    Mt, Mc = lr.scaling(A, d)
    assert np.array_equal(Mt, [4.0, 4e-8, 4e-8]) and np.array_equal(Mc, [2.0, 2e-8])
    Mt, Mc = lr.scaling(np.zeros((2, 2)), np.zeros(3))
    assert np.array_equal(Mt, [1.0, 1.0]) and np.array_equal(Mc, [1.0, 1.0, 1.0])
    assert np.array_equal(lr.scaling(np.zeros((2, 2)), np.zeros(1), n_lambda=0.5)[0], [0.5, 0.5])


def test_damping_ladder():
    assert np.array_equal(lr.ladder(0.9, 1), [0.9 / 5.0])
    assert np.array_equal(lr.ladder(0.9, 4), [0.9 / 5.0, 0.9, 0.9 * 5.0, 0.9 * 25.0])
    assert lr.ladder(1e15, 3)[-1] == 1e15 and lr.ladder(1e-15, 2)[0] == 1e-15


def test_loop_converges_and_its_trace_is_monotone():
    theta, c = _start()
    res = lr.lm_loop(_info, _grad, _losses, _loss, theta, c, n_subjects=N, max_iters=20, n_trials=4)
    tr = res["trace"]
    assert np.all(np.diff(tr) <= 0.0) and tr[-1] <= 1e-24 * tr[0]
    one = lr.lm_loop(_info, _grad, _losses, _loss, theta, c, n_subjects=N, max_iters=40, n_trials=1)
    assert one["trace"][-1] <= 1e-20 * tr[0]
    # a rejected iteration leaves the point and the loss alone and raises the damping 25-fold above the last rung
    rej = lr.lm_loop(_info, _grad, lambda t, cc: np.full(len(t), np.inf), _loss, theta, c, n_subjects=N, max_iters=2, n_trials=3)
    assert np.array_equal(rej["theta"], theta) and np.array_equal(rej["trace"], [tr[0]] * 3)
    assert np.allclose(rej["mu"], [1e-2, 25 * 5 * 1e-2, 25 * 5 * 25 * 5 * 1e-2], rtol=1e-15)
    far = lr.lm_loop(_info, _grad, lambda t, cc: np.full(len(t), np.inf), _loss, theta, c, n_subjects=N, max_iters=50, mu0=1e12)
    assert far["status"] == lr.STALLED and far["mu"][-1] == lr.MU_MAX
    done = lr.lm_loop(_info, _grad, _losses, _loss, res["theta"], res["c"], n_subjects=N, gtol=1e-9)
    assert done["status"] == lr.GRAD and done["n_iters"] == 0


def test_status_names_are_exported():
    from cude import _lib, api
    assert api.LM_STATUS == lr.STATUS_NAMES
    header = open(os.path.join(ROOT, "include", "cude.h")).read()
    codes = dict(re.findall(r"#define CUDE_LM_(\w+) (\d+)", header))
    assert [int(codes[n.upper()]) for n in api.LM_STATUS] == [0, 1, 2, 3, 4]
    assert (_lib.LM_GRAD, _lib.LM_DECREASE, _lib.LM_STALLED, _lib.LM_MAX_ITERS, _lib.LM_FAILED) == (0, 1, 2, 3, 4)
    assert (lr.GRAD, lr.DECREASE, lr.STALLED, lr.MAX_ITERS, lr.FAILED) == (0, 1, 2, 3, 4)
    assert {"cude_lm_candidates", "cude_train_lm"} <= set(_lib.exported_symbols())
