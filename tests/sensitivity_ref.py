"""Reference values for cude_sensitivity, from the oracle as it stands (oracle/cude_oracle.py): its forward solves run on
complex128 with the conditional parameter perturbed by i*1e-30, so that Im(u) / 1e-30 is d u / d cond to machine
precision (complex step: no subtraction).  Every subject is perturbed at once -- subjects do not interact, so column i
of the result is the derivative with respect to subject i's own parameter.  A second, independent route (torch autograd of
the same functions) is here for tests/test_sensitivity_host.py, which checks the two against each other.

Adaptive mode: the device's own accepted steps (cude_adaptive_steps) are replayed in complex arithmetic
(cude_oracle.replay_steps), as cpep_replay_loss_grad / supp_replay_loss_grad do for the adjoint."""
import numpy as np

import cude_oracle as o

H = 1e-30


def _stack(traj, N):
    """list over T of list over states of (N,) arrays / scalars -> complex array (n_state, T, N)."""
    return np.array([[np.broadcast_to(np.asarray(traj[ti][s], dtype=np.complex128), (N,)) for ti in range(len(traj))]
                     for s in range(len(traj[0]))])


def _summaries(u, obs_stn, w2):
    """u: complex (n_obs_states, T, N) of the OBSERVED states; obs_stn: their data (same shape); w2: weight^2 per state.
    Returns (info, score, sse) per subject."""
    sens, r = u.imag / H, u.real - obs_stn
    w2 = np.asarray(w2, dtype=np.float64)[:, None, None]
    return (w2 * sens ** 2).sum(axis=(0, 1)), (w2 * r * sens).sum(axis=(0, 1)), (w2 * r ** 2).sum(axis=(0, 1))


# ----------------------------------------------------------------------------- fixed step
def cpep_sens(nn, cond, pop, arch, n_steps, n_state=2, cond_space="log"):
    """(sens (n_state, T, N), info, score, sse) of the fixed-step c-peptide solve."""
    c = np.asarray(cond, dtype=np.complex128) + 1j * H
    u = _stack(o.cpep_forward(np, np.asarray(nn, dtype=np.float64), c, pop, arch, n_steps, n_state, cond_space), pop.N)
    info, score, sse = _summaries(u[:1], pop.cpeptide.T[None], [1.0])
    return u.imag / H, info, score, sse


def supp_sens(nn, theta, data, timepoints, arch, n_steps):
    """(sens (3, T, N), info, score, sse) of the fixed-step suppression solve, in suppression_loss's weighting."""
    c = np.asarray(theta, dtype=np.complex128) + 1j * H
    u = _stack(o.supp_forward(np, np.asarray(nn, dtype=np.float64), c, data, timepoints, arch, n_steps), data.shape[2])
    info, score, sse = _summaries(u, data, 1.0 / o.supp_scale(data) ** 2)
    return u.imag / H, info, score, sse


# ----------------------------------------------------------------------------- the same by torch autograd
def _torch_sens(forward, cond, n_state, T):
    import torch
    c = torch.tensor(np.asarray(cond, dtype=np.float64), requires_grad=True)
    traj = forward(c)
    sens = np.zeros((n_state, T, len(cond)))
    for s in range(n_state):
        for ti in range(T):
            v = traj[ti][s]
            if not (torch.is_tensor(v) and v.requires_grad):
                continue
            (g,) = torch.autograd.grad(v.sum(), c, retain_graph=True, allow_unused=True)
            if g is not None:
                sens[s, ti] = g.numpy()
    return sens


def cpep_sens_torch(nn, cond, pop, arch, n_steps, n_state=2, cond_space="log"):
    import torch
    return _torch_sens(lambda c: o.cpep_forward(torch, np.asarray(nn, dtype=np.float64), c, pop, arch, n_steps, n_state,
                                                cond_space), cond, n_state, pop.T)


def supp_sens_torch(nn, theta, data, timepoints, arch, n_steps):
    import torch
    return _torch_sens(lambda c: o.supp_forward(torch, np.asarray(nn, dtype=np.float64), c, data, timepoints, arch, n_steps),
                       theta, 3, len(timepoints))


# ----------------------------------------------------------------------------- adaptive: replay of given step sequences
def cpep_sens_replay(nn, cond, pop, arch, steps, cond_space="log"):
    """steps[i] = [(t_n, dt_n)] of subject i.  Returns (sens (2, T, N), info, score, sse)."""
    nn = [float(v) for v in nn]
    tpl = [float(v) for v in pop.timepoints]
    u = np.zeros((2, pop.T, pop.N), dtype=np.complex128)
    for i in range(pop.N):
        cb = complex(cond[i]) + 1j * H
        cb = np.exp(cb) if cond_space == "log" else cb
        c0 = float(pop.c0[i])
        G = [float(v) for v in pop.glucose[i]]
        k0, k1, k2, age = float(pop.k0[i]), float(pop.k1[i]), float(pop.k2[i]), float(pop.age[i])

        def rhs(t, y):
            dG = o.linear_interp(tpl, G, t) - G[0]
            if arch[1] == 0:
                prod = (nn[0] * dG) / (dG + cb) if dG >= 0 else 0.0 * cb
            elif pop.covariate:
                prod = o.mlp(np, [dG, cb, age], nn, arch) - o.mlp(np, [0.0, cb, age], nn, arch)
            else:
                prod = o.mlp(np, [dG, cb], nn, arch) - o.mlp(np, [0.0, cb], nn, arch)
            return [-(k0 + k2) * y[0] + k1 * y[1] + k0 * c0 + prod, -k1 * y[1] + k2 * y[0]]
        out = o.replay_steps(rhs, [c0 + 0.0 * cb, (k2 / k1) * c0 + 0.0 * cb], tpl, steps[i])
        assert out is not None, i
        u[:, :, i] = np.array(out, dtype=np.complex128).T
    info, score, sse = _summaries(u[:1], pop.cpeptide.T[None], [1.0])
    return u.imag / H, info, score, sse


def supp_sens_replay(nn, theta, data, timepoints, arch, steps):
    nn = [float(v) for v in nn]
    tpl = [float(v) for v in timepoints]
    N = data.shape[2]
    u = np.zeros((3, len(tpl), N), dtype=np.complex128)
    for i in range(N):
        cb = np.exp(complex(theta[i]) + 1j * H)
        out = o.replay_steps(lambda t, y: o.supp_rhs(np, nn, cb, arch, t, y),
                             [float(data[s, 0, i]) + 0.0 * cb for s in range(3)], tpl, steps[i])
        assert out is not None, i
        u[:, :, i] = np.array(out, dtype=np.complex128).T
    info, score, sse = _summaries(u, data, 1.0 / o.supp_scale(data) ** 2)
    return u.imag / H, info, score, sse
