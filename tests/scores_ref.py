"""Restatements for cude_subject_scores (the numbered rules in include/cude.h) and the per-subject oracle gradients its
rows are held to.

  fold            rule 2 / 3 in numpy: sets strictly in set order, s = s + (w * row) with the product rounded, then the sum
                  (numpy never contracts), sets with w == 0 skipped, bad sets counted.
  *_rows_torch    fixed-step rows: torch autograd of sse[i] through the oracle's own discretisation (cude_oracle.cpep_loss /
                  supp_loss).  Subjects do not interact, and cude_oracle.mlp reads its parameters entry by entry, so every
                  subject is given its OWN copy of the parameters (a (P, N) leaf: p[q] is then the (N,) vector of the
                  subjects' copies) and ONE backward pass of sum_i sse[i] leaves d sse[i] / d (copy i) in column i -- the
                  Jacobian that N backward passes over a shared vector give (rows_one_by_one; tests/test_scores_host.py
                  holds the two to each other), at 1/N of the time (N = 70: 1.3 s against 90 s).
  *_rows_replay   adaptive rows: the oracle's complex-step derivative of a GIVEN accepted-step sequence (cude_oracle.
                  *_replay_loss_grad on the one-subject population of subject i; the loss of one subject is its SSE).
  marginal_*      the marginal log-likelihood of a rule on given points as ONE torch graph, for Fisher's identity.
"""
import math

import numpy as np

import cude_oracle as o


def fold(rows, sse, w=None):
    """rows (K, N, P), sse (K, N), w (K, N) or None -> (s (N, P), wsse (N,), bad (N,) int32)"""
    rows, sse = np.asarray(rows, dtype=np.float64), np.asarray(sse, dtype=np.float64)
    K, N, P = rows.shape
    s, ws, bad = np.zeros((N, P)), np.zeros(N), np.zeros(N, dtype=np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            wk = np.ones(N) if w is None else np.asarray(w[k], dtype=np.float64)
            on = wk != 0.0
            prod = wk[:, None] * rows[k]
            s = np.where(on[:, None], s + prod, s)
            ws = np.where(on, ws + wk * sse[k], ws)
            bad += (on & ~(np.isfinite(sse[k]) & np.isfinite(rows[k]).all(axis=1))).astype(np.int32)
    return s, ws, bad


def finish(s, ws, bad, mask=None):
    """rule 3 / 4: (scores, wsse, failed) -- NaN rows of failed subjects, masked entries exactly 0"""
    failed = (bad > 0) | ~np.isfinite(ws) | ~np.isfinite(s).all(axis=1)
    out = np.where(failed[:, None], np.nan, s)
    if mask is not None:
        m = np.asarray(mask, dtype=np.float64)
        out = np.where(m[None, :] == 0.0, 0.0, out * m[None, :])
    return out, np.where(failed, np.nan, ws), failed


def exact_sum_cross(scores):
    """math.fsum over the rows that are not NaN: (sum (P,), cross (P, P), abs-sum (P,), abs-cross (P, P))"""
    ok = ~np.isnan(scores).any(axis=1)
    s = scores[ok]
    P = s.shape[1]
    tot = np.array([math.fsum(s[:, q]) for q in range(P)])
    cross = np.array([[math.fsum(s[:, q] * s[:, r]) for r in range(P)] for q in range(P)])
    return tot, cross, np.abs(s).sum(axis=0), np.abs(s).T @ np.abs(s)


# ----------------------------------------------------------------------------- fixed-step rows (torch autograd)
def _copies(nn, N):
    import torch
    return torch.tensor(np.repeat(np.asarray(nn, dtype=np.float64)[:, None], N, axis=1), requires_grad=True)


def _rows(sse, nn_b):
    sse.sum().backward()
    return nn_b.grad.numpy().T.copy(), sse.detach().numpy().copy()


def rows_one_by_one(sse, nn_t, subjects):
    """d sse[i] / d nn_t for a SHARED parameter vector nn_t, one backward pass per subject"""
    import torch
    return np.stack([torch.autograd.grad(sse[i], nn_t, retain_graph=True)[0].numpy().copy() for i in subjects])


def cpep_rows_torch(c, arch, cond=None, n_steps=30, cond_space="log"):
    """(rows (N, P), sse (N,)) of a conftest.make_cpep_case population at the conditionals `cond` (None: c["beta"]);
    arch may carry activation names (cude_oracle.general_arch); the symbolic model: arch = (1, 0, 0), nn = [p0]"""
    import torch
    pop = o.CPepPopulation(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"], covariate=(arch[0] == 3))
    nn_b = _copies(c["nn"], pop.N)
    be = torch.tensor(np.asarray(c["beta"] if cond is None else cond, dtype=np.float64))
    return _rows(o.cpep_loss(torch, nn_b, be, pop, arch, n_steps, 2, cond_space)[1], nn_b)


def supp_rows_torch(c, arch, cond=None, n_steps=30):
    import torch
    nn_b = _copies(c["nn"], c["data"].shape[2])
    th = torch.tensor(np.asarray(c["theta"] if cond is None else cond, dtype=np.float64))
    return _rows(o.supp_loss(torch, nn_b, th, c["data"], c["tp"], arch, n_steps, 0.0)[1], nn_b)


# ----------------------------------------------------------------------------- adaptive rows (step replay)
def cpep_rows_replay(c, arch, steps, cond=None, cond_space="log"):
    """steps[i] = [(t_n, dt_n)] of subject i -> (rows (N, P), sse (N,)): one-subject populations, whose loss IS the SSE"""
    cond = np.asarray(c["beta"] if cond is None else cond, dtype=np.float64)
    rows, sse = [], []
    for i in range(len(steps)):
        one = slice(i, i + 1)
        pop = o.CPepPopulation(c["tp"], c["G"][one], c["obs"][one], c["age"][one], c["t2dm"][one], covariate=(arch[0] == 3))
        loss, g, _, _ = o.cpep_replay_loss_grad(c["nn"], cond[one], pop, arch, [steps[i]], cond_space)
        rows.append(g)
        sse.append(loss)
    return np.array(rows), np.array(sse)


def supp_rows_replay(c, arch, steps, cond=None):
    """... the suppression model: the body of cude_oracle.supp_replay_loss_grad per subject (lam = 0), with the residuals
    scaled by the WHOLE population's scale as the population loss scales them (a one-subject population would have its own)"""
    cond = np.asarray(c["theta"] if cond is None else cond, dtype=np.float64)
    nn = np.asarray(c["nn"], dtype=np.float64)
    P, data = len(nn), c["data"]
    tpl = [float(v) for v in c["tp"]]
    scale = o.supp_scale(data)
    rows, sse = [], []
    for i in range(len(steps)):
        pb, cb = o._complex_step_batch(nn, cond[i])
        out = o.replay_steps(lambda t, u: o.supp_rhs(np, pb, cb, arch, t, u), [float(data[s, 0, i]) + 0.0 * cb for s in range(3)],
                             tpl, steps[i])
        e = 0.0 * cb
        for ti in range(1, len(tpl)):
            for s in range(3):
                e = e + ((out[ti][s] - data[s, ti, i]) / scale[s]) ** 2
        rows.append(e.imag[:P] / 1e-30)
        sse.append(e[0].real)
    return np.array(rows), np.array(sse)


# ----------------------------------------------------------------------------- the marginal likelihood as one graph
def log_weight_terms(torch, sse, x, a_k, T, sigma, prior_mean, prior_sd):
    """t_ik = a_k + ll_ik + lp_ik for one node (include/cude.h, cude_marginal_likelihood rule 2)"""
    ll = -(T / 2.0) * math.log(sigma * sigma) - sse / (2.0 * sigma * sigma)
    u = (x - prior_mean) / prior_sd
    lp = -0.5 * u * u - math.log(prior_sd) - 0.5 * math.log(2.0 * math.pi)
    return a_k + ll + lp


def marginal_cpep_torch(c, arch, points, log_weights, sigma, prior_mean, prior_sd, n_steps=30):
    """total = sum_i logsumexp_k t_ik at the points (K, N) through cude_oracle.cpep_loss as one torch graph.  Returns
    dict(total, gradient (P,) = autograd of total, rows (K, N, P), sse (K, N), w (K, N) = the posterior weights)."""
    import torch
    pop = o.CPepPopulation(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"], covariate=(arch[0] == 3))
    nn_t = torch.tensor(np.asarray(c["nn"], dtype=np.float64), requires_grad=True)
    K = len(log_weights)
    sses, terms = [], []
    for k in range(K):
        x = torch.tensor(np.asarray(points[k], dtype=np.float64))
        _, sse = o.cpep_loss(torch, nn_t, x, pop, arch, n_steps, 2)
        sses.append(sse)
        terms.append(log_weight_terms(torch, sse, x, float(log_weights[k]), pop.T, sigma, prior_mean, prior_sd))
    t = torch.stack(terms)
    total = torch.logsumexp(t, dim=0).sum()
    grad = torch.autograd.grad(total, nn_t, retain_graph=True)[0].numpy().copy()
    rows = np.stack([rows_one_by_one(s, nn_t, range(pop.N)) for s in sses])
    w = torch.softmax(t, dim=0).detach().numpy().copy()
    return dict(total=float(total.detach()), gradient=grad, rows=rows, sse=np.stack([s.detach().numpy() for s in sses]), w=w,
                terms=t.detach().numpy().copy())
