"""Reference values for cude_curvature, from the oracle as it stands (oracle/cude_oracle.py), by two CPU routes:

  (a) torch double backward through cude_oracle.cpep_forward(torch, ...) / supp_forward(torch, ...): exact to rounding,
      also across relu kinks (torch takes relu'' = 0 and relu' = 0 at the kink, the device's convention); 2-14 s per case.
  (b) a central-difference stencil in the conditional parameter over tests/sensitivity_ref.py's complex-step FIRST
      derivatives: 0.2-0.4 s per case.  The first derivatives carry no subtraction error, so only one order is differenced.
      Adaptive mode: the same over *_sens_replay at the device's own accepted steps of the centre point -- which holds the
      steps fixed, the convention being tested (the second derivative of the accepted-step map).

Every subject is perturbed at once: subjects do not interact, so column i is the derivative with respect to subject i's
own parameter.  tests/test_curvature_host.py holds (b) to (a) at a tenth of the device's bar, and shows that (b) is wrong by
orders of magnitude with relu (the stencil straddles kinks): relu cases take route (a) only.

The stencil is the 6th-order one at h = 2e-4: truncation h^6 f^(7) / 140 of the differentiated function, rounding
~ 1.5 eps / h ~ 2e-12.  (The 4th-order stencil at h = 1e-4 met 1e-10 on every case but supp 3x5 tanh / identity, 4.3e-10;
this one measured 4e-12 ... 2e-11 against route (a) on the cases scanned, 3.6e-10 on that case at h = 5e-4 and 2.3e-8 at
h = 1e-3, where truncation takes over.)"""
import numpy as np

import cude_oracle as o
import sensitivity_ref as sref

STENCIL_H = 2e-4
# f'(x) ~ sum_k c_k f(x + k h) / h, k = -3 ... 3
STENCIL = ((-3, -1.0 / 60.0), (-2, 3.0 / 20.0), (-1, -3.0 / 4.0), (1, 3.0 / 4.0), (2, -3.0 / 20.0), (3, 1.0 / 60.0))


def _finish(sens, sens2, info, score, sse, resid, w2, obs_rows):
    """curv = info + sum w^2 r d2yhat; returns dict with the pieces (second = the second-order sum alone)."""
    w2 = np.asarray(w2, dtype=np.float64)[:, None, None]
    second = (w2 * resid * sens2[obs_rows]).sum(axis=(0, 1))
    return dict(sens=sens, sens2=sens2, curv=info + second, info=info, score=score, sse=sse, second=second)


def _stencil(first, cond, h=STENCIL_H):
    """first(cond) -> sens array; returns d sens / d cond by the stencil (all subjects at once)."""
    cond = np.asarray(cond, dtype=np.float64)
    acc = None
    for k, ck in STENCIL:
        v = ck * first(cond + k * h)
        acc = v if acc is None else acc + v
    return acc / h


# ----------------------------------------------------------------------------- route (b), fixed step
def cpep_curv(nn, cond, pop, arch, n_steps, n_state=2, cond_space="log", h=STENCIL_H):
    sens, info, score, sse = sref.cpep_sens(nn, cond, pop, arch, n_steps, n_state, cond_space)
    sens2 = _stencil(lambda c: sref.cpep_sens(nn, c, pop, arch, n_steps, n_state, cond_space)[0], cond, h)
    sens2[:, 0] = 0.0                                          # u(t_0) depends on no parameter
    u = sref._stack(o.cpep_forward(np, np.asarray(nn, dtype=np.float64), np.asarray(cond, dtype=np.float64), pop, arch,
                                   n_steps, n_state, cond_space), pop.N).real
    return _finish(sens, sens2, info, score, sse, u[:1] - pop.cpeptide.T[None], [1.0], slice(0, 1))


def supp_curv(nn, theta, data, timepoints, arch, n_steps, h=STENCIL_H):
    sens, info, score, sse = sref.supp_sens(nn, theta, data, timepoints, arch, n_steps)
    sens2 = _stencil(lambda c: sref.supp_sens(nn, c, data, timepoints, arch, n_steps)[0], theta, h)
    sens2[:, 0] = 0.0
    sens2[0] = 0.0                                             # state 1 depends on no parameter
    u = sref._stack(o.supp_forward(np, np.asarray(nn, dtype=np.float64), np.asarray(theta, dtype=np.float64), data,
                                   timepoints, arch, n_steps), data.shape[2]).real
    return _finish(sens, sens2, info, score, sse, u - data, 1.0 / o.supp_scale(data) ** 2, slice(0, 3))


# ----------------------------------------------------------------------------- route (b), adaptive: the steps held fixed
def supp_curv_replay(nn, theta, data, timepoints, arch, steps, h=STENCIL_H):
    sens, info, score, sse = sref.supp_sens_replay(nn, theta, data, timepoints, arch, steps)
    sens2 = _stencil(lambda c: sref.supp_sens_replay(nn, c, data, timepoints, arch, steps)[0], theta, h)
    sens2[:, 0] = 0.0
    sens2[0] = 0.0
    w2 = 1.0 / o.supp_scale(data) ** 2
    # (sensitivity_ref's replay does not return the residuals: they come from a real replay of the same steps)
    resid = _replay_resid_supp(nn, theta, data, timepoints, arch, steps)
    return _finish(sens, sens2, info, score, sse, resid, w2, slice(0, 3))


def _cpep_replay_real(nn, cond, pop, arch, steps, cond_space):
    """Real parts of the replayed trajectory, (2, T, N): sensitivity_ref's replay with its outputs kept."""
    nnl = [float(v) for v in nn]
    tpl = [float(v) for v in pop.timepoints]
    u = np.zeros((2, pop.T, pop.N))
    for i in range(pop.N):
        cb = float(np.exp(cond[i])) if cond_space == "log" else float(cond[i])
        c0 = float(pop.c0[i])
        G = [float(v) for v in pop.glucose[i]]
        k0, k1, k2, age = float(pop.k0[i]), float(pop.k1[i]), float(pop.k2[i]), float(pop.age[i])

        def rhs(t, y):
            dG = o.linear_interp(tpl, G, t) - G[0]
            if arch[1] == 0:
                prod = (nnl[0] * dG) / (dG + cb) if dG >= 0 else 0.0
            elif pop.covariate:
                prod = o.mlp(np, [dG, cb, age], nnl, arch) - o.mlp(np, [0.0, cb, age], nnl, arch)
            else:
                prod = o.mlp(np, [dG, cb], nnl, arch) - o.mlp(np, [0.0, cb], nnl, arch)
            return [-(k0 + k2) * y[0] + k1 * y[1] + k0 * c0 + prod, -k1 * y[1] + k2 * y[0]]
        out = o.replay_steps(rhs, [c0, (k2 / k1) * c0], tpl, steps[i])
        assert out is not None, i
        u[:, :, i] = np.array(out, dtype=np.float64).T
    return u


def cpep_curv_replay(nn, cond, pop, arch, steps, cond_space="log", h=STENCIL_H):
    sens, info, score, sse = sref.cpep_sens_replay(nn, cond, pop, arch, steps, cond_space)
    sens2 = _stencil(lambda c: sref.cpep_sens_replay(nn, c, pop, arch, steps, cond_space)[0], cond, h)
    sens2[:, 0] = 0.0
    u = _cpep_replay_real(nn, np.asarray(cond, dtype=np.float64), pop, arch, steps, cond_space)
    return _finish(sens, sens2, info, score, sse, u[:1] - pop.cpeptide.T[None], [1.0], slice(0, 1))


def _replay_resid_supp(nn, theta, data, timepoints, arch, steps):
    import math
    nnl = [float(v) for v in nn]
    tpl = [float(v) for v in timepoints]
    N = data.shape[2]
    u = np.zeros((3, len(tpl), N))
    for i in range(N):
        et = math.exp(float(theta[i]))
        out = o.replay_steps(lambda t, y: o.supp_rhs(np, nnl, et, arch, t, y), [float(data[s, 0, i]) for s in range(3)], tpl,
                             steps[i])
        assert out is not None, i
        u[:, :, i] = np.array(out, dtype=np.float64).T
    return u - data


# ----------------------------------------------------------------------------- route (a): torch double backward
def _torch_jet(forward, cond, n_state, T):
    """(u, sens, sens2), each (n_state, T, N): values, first and second derivative of every output with respect to its
    own subject's parameter (the Hessian of output i is diagonal: it depends on cond_i alone)."""
    import torch
    c = torch.tensor(np.asarray(cond, dtype=np.float64), requires_grad=True)
    traj = forward(c)
    N = len(cond)
    u, sens, sens2 = (np.zeros((n_state, T, N)) for _ in range(3))
    for s in range(n_state):
        for ti in range(T):
            v = traj[ti][s]
            if torch.is_tensor(v):
                u[s, ti] = v.detach().numpy()
            else:
                u[s, ti] = np.asarray(v, dtype=np.float64)
            if not (torch.is_tensor(v) and v.requires_grad):
                continue
            (g,) = torch.autograd.grad(v.sum(), c, create_graph=True, allow_unused=True)
            if g is None:
                continue
            sens[s, ti] = g.detach().numpy()
            if g.requires_grad:
                (g2,) = torch.autograd.grad(g.sum(), c, retain_graph=True, allow_unused=True)
                if g2 is not None:
                    sens2[s, ti] = g2.numpy()
    return u, sens, sens2


def _from_jet(u, sens, sens2, obs, w2, rows):
    w = np.asarray(w2, dtype=np.float64)[:, None, None]
    r = u[rows] - obs
    info = (w * sens[rows] ** 2).sum(axis=(0, 1))
    score = (w * r * sens[rows]).sum(axis=(0, 1))
    sse = (w * r ** 2).sum(axis=(0, 1))
    return _finish(sens, sens2, info, score, sse, r, w2, rows)


def cpep_curv_torch(nn, cond, pop, arch, n_steps, n_state=2, cond_space="log"):
    import torch
    jet = _torch_jet(lambda c: o.cpep_forward(torch, np.asarray(nn, dtype=np.float64), c, pop, arch, n_steps, n_state,
                                              cond_space), cond, n_state, pop.T)
    return _from_jet(*jet, pop.cpeptide.T[None], [1.0], slice(0, 1))


def supp_curv_torch(nn, theta, data, timepoints, arch, n_steps):
    import torch
    jet = _torch_jet(lambda c: o.supp_forward(torch, np.asarray(nn, dtype=np.float64), c, data, timepoints, arch, n_steps),
                     theta, 3, len(timepoints))
    return _from_jet(*jet, data, 1.0 / o.supp_scale(data) ** 2, slice(0, 3))


# ----------------------------------------------------------------------------- what api.py builds from the curvature
def observed_se(curv, sigma):
    """sigma / sqrt(curv) where curv > 0, inf where curv <= 0, NaN for a failed subject (NaN curvature)."""
    curv = np.asarray(curv, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(np.isnan(curv), np.nan, np.where(curv > 0, sigma / np.sqrt(np.where(curv > 0, curv, 1.0)), np.inf))


def map_classes(curv, info, pw):
    """(curv + pw, info + pw, ratio, class) per subject: 'minimum', 'not_a_minimum' (curv + pw <= 0), 'failed' (NaN)."""
    a, b = np.asarray(curv) + pw, np.asarray(info) + pw
    cls = np.where(np.isnan(a), "failed", np.where(a > 0, "minimum", "not_a_minimum"))
    with np.errstate(all="ignore"):
        return a, b, a / b, cls
