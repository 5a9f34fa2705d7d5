"""Host restatement of the Levenberg-Marquardt rule of cude_lm_candidates / cude_train_lm (include/cude.h), in numpy and by
another route: the step comes from numpy.linalg.solve on the dense (P + N) system, not from elimination.  The problem enters
through four callables, so that the same loop runs on the device's entry points (tests/test_gpu_lm.py), on the CPU oracles and
on a synthetic arrowhead problem (tests/test_lm_host.py):

    info(theta, c)            -> A (P, P), B (P, N) with column i = b_i, d (N,)       (penalty weight 0)
    grad(theta, c)            -> loss, g_theta (P,), g_c (N,)                         (the LOSS's gradient: 2 / N of ghat)
    losses(thetas, cs)        -> (K,) trial losses of K parameter sets
    forward(theta, c)         -> the loss that the trace carries
"""
import numpy as np

GRAD, DECREASE, STALLED, MAX_ITERS, FAILED = range(5)
STATUS_NAMES = ("grad", "decrease", "stalled", "max_iters", "failed")
FLOOR, MU_MIN, MU_MAX = 1e-8, 1e-15, 1e15


RATIO = 5.0                                 # between the rungs of the damping ladder


def ladder(mu, K):
    """mu_k = mu RATIO^(k - 1), k = 0 ... K - 1, clamped"""
    out = [mu / RATIO]
    f = 1.0
    for _ in range(1, K):
        out.append(mu * f)
        f *= RATIO
    return np.clip(np.array(out), MU_MIN, MU_MAX)


def scaling(A, d, n_lambda=0.0):
    """(M_theta (P,), M_c (N,)): the diagonal, floored at 1e-8 of its maximum; 1 where that maximum is not > 0"""
    a = np.diag(A) + n_lambda
    ma, md = max(0.0, np.max(a)), max(0.0, np.max(d))
    return (np.maximum(a, FLOOR * ma) if ma > 0.0 else np.ones_like(a),
            np.maximum(d, FLOOR * md) if md > 0.0 else np.ones_like(d))


def dense_system(A, B, d, n_lambda=0.0, mask=None):
    """H (P + N, P + N) = [[A + N lambda I, B], [B^T, D]] and M's diagonal; a masked parameter's row and column of H are the
    unit diagonal (its right-hand side is the caller's to zero)"""
    P, N = B.shape
    H = np.zeros((P + N, P + N))
    H[:P, :P] = A + n_lambda * np.eye(P)
    H[:P, P:] = B
    H[P:, :P] = B.T
    H[P:, P:] = np.diag(d)
    M = np.concatenate(scaling(A, d, n_lambda))
    if mask is not None:
        for q in np.flatnonzero(np.asarray(mask) == 0.0):
            H[q, :] = 0.0
            H[:, q] = 0.0
            H[q, q] = 1.0
            M[q] = 0.0
    return H, M


def dense_step(H, M, ghat, mu):
    return np.linalg.solve(H + mu * np.diag(M), -ghat)


def eliminated_step(A, B, d, ghat, mu, n_lambda=0.0):
    """the same step by the device's route: Schur complement, Cholesky, back-substitution"""
    P, N = B.shape
    Mt, Mc = scaling(A, d, n_lambda)
    e = d + mu * Mc
    S = A + n_lambda * np.eye(P) + mu * np.diag(Mt) - (B / e) @ B.T
    rhs = -(ghat[:P] - B @ (ghat[P:] / e))
    L = np.linalg.cholesky(S)
    dth = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
    dc = -(ghat[P:] + B.T @ dth) / e
    return np.concatenate([dth, dc])


def pred_terms(ghat, M, delta, mu):
    """the terms of pred = -ghat^T delta + mu delta^T M delta"""
    return np.concatenate([-ghat * delta, mu * M * delta * delta])


def backward_error(H, M, ghat, mu, delta):
    """eta = |(H + mu M) delta + ghat|_inf / (|H + mu M|_inf |delta|_inf + |ghat|_inf)"""
    K = H + mu * np.diag(M)
    r = K @ delta + ghat
    return np.max(np.abs(r)) / (np.max(np.sum(np.abs(K), axis=1)) * np.max(np.abs(delta)) + np.max(np.abs(ghat)))


def eta_bar(N, P):
    """2^-52 (N + 4 P (3 P + 1)): the a-priori normwise backward-error bound of a Cholesky solve of order P, plus one rounding
    per subject of the elimination sums"""
    return 2.0 ** -52 * (N + 4 * P * (3 * P + 1))


def lm_loop(info, grad, losses, forward, theta, c, *, n_subjects, lam=0.0, max_iters=20, n_trials=4, mu0=1e-2, gtol=0.0,
            ftol=0.0, mask=None, visit=None):
    """The loop of cude_train_lm.  visit(it, theta, c, mu): called at the point every iteration starts from.  Returns
    dict(theta, c, trace, mu, n_iters, status)."""
    theta, c = np.array(theta, dtype=np.float64), np.array(c, dtype=np.float64)
    P = theta.size
    mu = float(np.clip(mu0, MU_MIN, MU_MAX))
    F = forward(theta, c)
    trace, mus = [F], [mu]
    status = MAX_ITERS if np.isfinite(F) else FAILED
    it = 0
    while status == MAX_ITERS and it < max_iters:
        if visit is not None:
            visit(it, theta, c, mu)
        loss, g_t, g_c = grad(theta, c)
        g = np.concatenate([g_t, g_c])
        if not np.isfinite(loss) or not np.all(np.isfinite(g)):
            status = FAILED
            break
        A, B, d = info(theta, c)
        if not (np.all(np.isfinite(A)) and np.all(np.isfinite(B)) and np.all(np.isfinite(d))):
            status = FAILED
            break
        if np.max(np.abs(g)) <= gtol:
            status = GRAD
            break
        it += 1
        ghat = 0.5 * n_subjects * g
        H, M = dense_system(A, B, d, n_subjects * lam, mask)
        mu_k = ladder(mu, n_trials)
        thetas, cs = [], []
        for m in mu_k:
            try:
                delta = dense_step(H, M, ghat, m)
            except np.linalg.LinAlgError:
                delta = np.full(ghat.shape, np.nan)
            ok = np.all(np.isfinite(delta))
            thetas.append(theta + delta[:P] if ok else theta.copy())
            cs.append(c + delta[P:] if ok else c.copy())
        f = np.asarray(losses(np.stack(thetas), np.stack(cs)), dtype=np.float64)
        best, fb = -1, F
        for k in range(n_trials):
            if np.isfinite(f[k]) and f[k] < fb:
                best, fb = k, f[k]
        Fn = forward(thetas[best], cs[best]) if best >= 0 else np.inf
        if best >= 0 and np.isfinite(Fn) and Fn < F:
            small = F - Fn <= ftol * F
            theta, c, F = thetas[best], cs[best], Fn
            mu = float(np.clip(mu_k[best] / RATIO, MU_MIN, MU_MAX))
            if small:
                status = DECREASE
        else:
            mu = RATIO * RATIO * mu_k[-1]
            if mu > MU_MAX:
                mu, status = MU_MAX, STALLED
        trace.append(F)
        mus.append(mu)
    return dict(theta=theta, c=c, trace=np.array(trace), mu=np.array(mus), n_iters=it, status=status)
