"""Restatements for cude_network_information (the numbered rules in include/cude.h) and the oracle Jacobians its rows are
held to.

  *_jac_torch     fixed-step rows: torch autograd of the oracle's own trajectories (cude_oracle.cpep_forward /
                  supp_forward).  Every subject is given its own copy of the parameters, as scores_ref does, so ONE batched
                  backward pass (one unit seed per live output, is_grads_batched) leaves d yhat_io / d (copy i) for all
                  subjects and outputs.
  *_jac_replay    adaptive rows: the complex-step derivative of cude_oracle.replay_steps over a GIVEN accepted-step
                  sequence, one subject at a time -- the outputs themselves instead of the loss scores_ref.*_rows_replay forms.
  out_weights     the loss's weights w_o per output.
  information     rules 3 - 7 in numpy: b, d (the fold, every operation rounded on its own), status, NaN rows, A, S, qform.
  exact_*         math.fsum forms of A and the Schur term with the sums of magnitudes the bars are built from.
"""
import math

import numpy as np

import cude_oracle as o

FAILED, FLAT = 1, 2


def out_weights(model, T, data=None):
    """(n_out,) loss weights: 1 for the c-peptide outputs, 1 / scale_s^2 for output s + 3 j of the suppression model"""
    if model != "supp":
        return np.ones(T)
    s = o.supp_scale(data)
    return np.tile(1.0 / (s * s), T)


def live_outputs(model, T):
    if model != "supp":
        return list(range(1, T))
    return [s + 3 * j for j in range(1, T) for s in (1, 2)]


# ----------------------------------------------------------------------------- fixed-step rows (torch autograd)
def _batched_jacobian(ys, nn_b, cond_t):
    """ys: list of (N,) outputs -> (J (N, L, P), jc (N, L))"""
    import torch
    Y = torch.stack(ys)                                           # (L, N)
    L, N = Y.shape
    seeds = torch.zeros(L, L, N, dtype=Y.dtype)
    for l in range(L):
        seeds[l, l, :] = 1.0
    g_nn, g_c = torch.autograd.grad(Y, [nn_b, cond_t], grad_outputs=seeds, is_grads_batched=True, allow_unused=True)
    J = g_nn.permute(2, 0, 1).numpy().copy()                      # (L, P, N) -> (N, L, P)
    jc = np.zeros((N, L)) if g_c is None else g_c.permute(1, 0).numpy().copy()
    return J, jc


def cpep_jac_torch(c, arch, cond=None, n_steps=30, cond_space="log", n_state=2):
    """(jac (N, T, P), jcond (N, T), traj (N, T)) of a conftest.make_cpep_case population: state 1 at the data's times"""
    import torch
    pop = o.CPepPopulation(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"], covariate=(arch[0] == 3))
    nn_b = sr_copies(c["nn"], pop.N)
    be = torch.tensor(np.asarray(c["beta"] if cond is None else cond, dtype=np.float64), requires_grad=True)
    traj = o.cpep_forward(torch, nn_b, be, pop, arch, n_steps, n_state, cond_space)
    T = pop.T
    J, jc = _batched_jacobian([traj[j][0] for j in range(1, T)], nn_b, be)
    jac, jcond = np.zeros((pop.N, T, J.shape[2])), np.zeros((pop.N, T))
    jac[:, 1:, :], jcond[:, 1:] = J, jc
    y = np.stack([(traj[j][0] + 0.0 * be).detach().numpy() for j in range(T)], axis=1)
    return jac, jcond, y


def supp_jac_torch(c, arch, cond=None, n_steps=30):
    """(jac (N, 3 T, P), jcond (N, 3 T), traj (N, 3 T)), output o = s + 3 j"""
    import torch
    data, T = c["data"], len(c["tp"])
    N = data.shape[2]
    nn_b = sr_copies(c["nn"], N)
    th = torch.tensor(np.asarray(c["theta"] if cond is None else cond, dtype=np.float64), requires_grad=True)
    traj = o.supp_forward(torch, nn_b, th, data, c["tp"], arch, n_steps)
    live = live_outputs("supp", T)
    J, jc = _batched_jacobian([traj[q // 3][q % 3] for q in live], nn_b, th)
    jac, jcond = np.zeros((N, 3 * T, J.shape[2])), np.zeros((N, 3 * T))
    jac[:, live, :], jcond[:, live] = J, jc
    y = np.stack([(traj[q // 3][q % 3] + 0.0 * th).detach().numpy() for q in range(3 * T)], axis=1)
    return jac, jcond, y


def sr_copies(nn, N):
    import torch
    return torch.tensor(np.repeat(np.asarray(nn, dtype=np.float64)[:, None], N, axis=1), requires_grad=True)


# ----------------------------------------------------------------------------- adaptive rows (step replay)
def cpep_jac_replay(c, arch, steps, cond=None, cond_space="log"):
    """steps[i] = [(t_n, dt_n)] of subject i -> (jac (N, T, P), jcond (N, T), traj (N, T)); the right-hand side is that of
    cude_oracle.cpep_replay_loss_grad"""
    cond = np.asarray(c["beta"] if cond is None else cond, dtype=np.float64)
    nn = np.asarray(c["nn"], dtype=np.float64)
    P, T = len(nn), len(c["tp"])
    pop = o.CPepPopulation(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"], covariate=(arch[0] == 3))
    tpl = [float(v) for v in pop.timepoints]
    jac, jcond, y = np.zeros((len(steps), T, P)), np.zeros((len(steps), T)), np.zeros((len(steps), T))
    for i in range(len(steps)):
        c0 = float(pop.c0[i])
        pb, cb = o._complex_step_batch(nn, cond[i], cond_space)
        G = [float(v) for v in pop.glucose[i]]
        k0, k1, k2, age = float(pop.k0[i]), float(pop.k1[i]), float(pop.k2[i]), float(pop.age[i])

        def rhs(t, u):
            dG = o.linear_interp(tpl, G, t) - G[0]
            if arch[1] == 0:
                prod = (pb[0] * dG) / (dG + cb) if dG >= 0 else 0.0 * cb
            elif pop.covariate:
                prod = o.mlp(np, [dG, cb, age], pb, arch) - o.mlp(np, [0.0, cb, age], pb, arch)
            else:
                prod = o.mlp(np, [dG, cb], pb, arch) - o.mlp(np, [0.0, cb], pb, arch)
            return [-(k0 + k2) * u[0] + k1 * u[1] + k0 * c0 + prod, -k1 * u[1] + k2 * u[0]]
        out = o.replay_steps(rhs, [c0 + 0.0 * cb, (k2 / k1) * c0 + 0.0 * cb], tpl, steps[i])
        for j in range(T):
            jac[i, j], jcond[i, j], y[i, j] = out[j][0].imag[:P] / 1e-30, out[j][0].imag[P] / 1e-30, out[j][0][0].real
    return jac, jcond, y


def supp_jac_replay(c, arch, steps, cond=None):
    cond = np.asarray(c["theta"] if cond is None else cond, dtype=np.float64)
    nn = np.asarray(c["nn"], dtype=np.float64)
    P, data = len(nn), c["data"]
    tpl = [float(v) for v in c["tp"]]
    T = len(tpl)
    jac, jcond, y = np.zeros((len(steps), 3 * T, P)), np.zeros((len(steps), 3 * T)), np.zeros((len(steps), 3 * T))
    for i in range(len(steps)):
        pb, cb = o._complex_step_batch(nn, cond[i])
        out = o.replay_steps(lambda t, u: o.supp_rhs(np, pb, cb, arch, t, u), [float(data[s, 0, i]) + 0.0 * cb for s in range(3)],
                             tpl, steps[i])
        for j in range(T):
            for s in range(3):
                v = out[j][s] + 0.0 * cb
                jac[i, s + 3 * j], jcond[i, s + 3 * j], y[i, s + 3 * j] = v.imag[:P] / 1e-30, v.imag[P] / 1e-30, v[0].real
    return jac, jcond, y


# ----------------------------------------------------------------------------- the rules in numpy
def information(J, jc, w, pw=0.0, mask=None, cov=None, profiled=False, bad=None):
    """J (N, n_out, P), jc (N, n_out), w (n_out,) -> dict(jac, jcond, coupling, dcond, status, gn, schur, qform) by rules 3 - 7;
    gn and schur by plain numpy sums (the device's order is its own: tests bound them with exact_*).  bad (N,) bool: subjects
    whose solve failed for a reason the rows do not show."""
    J, jc, w = np.array(J, dtype=np.float64), np.array(jc, dtype=np.float64), np.asarray(w, dtype=np.float64)
    N, n_out, P = J.shape
    raw_bad = ~(np.isfinite(J).all(axis=(1, 2)) & np.isfinite(jc).all(axis=1))
    if bad is not None:
        raw_bad |= np.asarray(bad, dtype=bool)
    m = np.ones(P) if mask is None else np.asarray(mask, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        Jm = np.where(m == 0.0, 0.0, J * m)
        b, d = np.zeros((N, P)), np.zeros(N)
        for q in range(n_out):
            wj = w[q] * jc[:, q]
            b = b + wj[:, None] * Jm[:, q]
            d = d + wj * jc[:, q]
        failed = raw_bad | ~np.isfinite(d) | ~np.isfinite(b).all(axis=1)
        den = d + pw
        flat = ~failed & ~(den > 0.0)
        ok = ~failed & ~flat
        t = np.where(ok[:, None] & (m != 0.0), b / np.sqrt(np.where(ok, den, 1.0))[:, None], 0.0)
        live = ~failed
        gn = np.einsum("o,ioq,ior->qr", w, Jm[live], Jm[live])
        schur = gn - t.T @ t
        out = dict(gn=gn, schur=schur, t=t, status=(failed * FAILED + flat * FLAT).astype(np.int32))
        nanrow = np.where(m == 0.0, 0.0, np.nan)
        out["jac"] = np.where(failed[:, None, None], nanrow[None, None, :], Jm)
        out["jcond"] = np.where(failed[:, None], np.nan, jc)
        out["coupling"] = np.where(failed[:, None], nanrow[None, :], b)
        out["dcond"] = np.where(failed, np.nan, d)
        if cov is not None:
            coef = np.where((ok if profiled else np.zeros(N, dtype=bool))[:, None], jc / np.where(ok, den, 1.0)[:, None], 0.0)
            z = Jm - coef[:, :, None] * np.where(failed[:, None], 0.0, b)[:, None, :]
            qf = np.einsum("ioq,qr,ior->io", z, np.asarray(cov, dtype=np.float64), z)
            out["qform"] = np.where(failed[:, None], np.nan, qf)
            out["z"] = z
    return out


def exact_gn(J, w, status):
    """math.fsum over the subjects that did not fail: (A (P, P), sum of |w J_q J_r| (P, P)); J as the device returned it"""
    ok = (np.asarray(status) & FAILED) == 0
    X = np.asarray(J)[ok]
    P = X.shape[2]
    Xw = X * np.asarray(w)[None, :, None]
    A = np.zeros((P, P))
    for q in range(P):
        for r in range(q, P):
            A[q, r] = A[r, q] = math.fsum((Xw[:, :, q] * X[:, :, r]).ravel())
    mag = np.einsum("ioq,ior->qr", np.abs(Xw), np.abs(X))
    return A, mag


def exact_schur_term(coupling, dcond, pw, status):
    """(sum_i b_i b_i^T / (d_i + pw) over the subjects that are neither failed nor flat by math.fsum, sum of |t_q| |t_r|)"""
    ok = np.asarray(status) == 0
    b, den = np.asarray(coupling)[ok], np.asarray(dcond)[ok] + pw
    P = b.shape[1]
    X = np.zeros((P, P))
    for q in range(P):
        for r in range(q, P):
            X[q, r] = X[r, q] = math.fsum(b[:, q] * b[:, r] / den)
    t = np.abs(b) / np.sqrt(den)[:, None]
    return X, t.T @ t
