"""cude_bootstrap_conditional restated in numpy from the rules' text (include/cude.h): the replicate data of rule 2, the
refits of rule 4 by tests/refine_ref.py's restatement of the fit over the CPU oracle's tangent solves, the summaries of rule
5 -- the yardstick of tests/test_gpu_bootstrap.py, which tests/test_bootstrap_host.py holds against numpy's own statistics.

Layouts.  yhat and the population's observations `pop`: (S, T, N), S = 1 for the c-peptide models (state 1) and 3 for the
suppression model.  Noise: (B, S * T, N), the device's [n_reps][rows][N].  Replicate data: (B, S, T, N).

The B replicates of N subjects are refitted as ONE population of B * N subjects (replicate-major): no quantity of
refine_ref.refine crosses subjects, so a subject's iteration is what a loop over the replicates would run.

Suppression model: refine_ref.supp_evaluator takes the loss weights 1 / scale^2 from the data it is given, which for a
replicate would be the replicate's own maxima; rule 2 keeps the population's weights, so supp_evaluator below is that
function with the weights passed in."""
import numpy as np

import refine_ref as rr


def replicate_data(yhat, sigma, scale, noise, pop):
    """Rule 2: y*[b, s, t, i] = yhat[s, t, i] + (sigma[i] scale[s]) eps[b, s, t, i], every operation rounded on its own; the
    rows of t_0 are the population's."""
    S, T, N = yhat.shape
    eps = np.asarray(noise, dtype=np.float64).reshape(-1, S, T, N)
    amp = np.asarray(sigma, dtype=np.float64)[None, None, None, :] * np.asarray(scale, dtype=np.float64)[None, :, None, None]
    y = yhat[None] + amp * eps
    y[:, :, 0, :] = pop[:, 0, :]
    return y


def cpep_yhat(c, center, n_steps=30, n_state=2, cond_space="log", nn=None, arch=None):
    """State 1 of the oracle's fixed-step solve at `center`: (1, T, N)."""
    import cude_oracle as o
    arch = c["arch"] if arch is None else arch
    nn = c["nn"] if nn is None else nn
    N = len(c["age"])
    pop = o.CPepPopulation(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"], covariate=(arch[0] == 3))
    traj = o.cpep_forward(np, np.asarray(nn, dtype=np.float64), np.asarray(center, dtype=np.float64), pop, arch, n_steps, n_state,
                          cond_space)
    return np.stack([np.broadcast_to(np.asarray(traj[t][0], dtype=np.float64), (N,)) for t in range(len(c["tp"]))])[None]


def supp_yhat(c, center, n_steps=30):
    import cude_oracle as o
    N = c["data"].shape[2]
    traj = o.supp_forward(np, np.asarray(c["nn"], dtype=np.float64), np.asarray(center, dtype=np.float64), c["data"], c["tp"],
                          c["arch"], n_steps)
    return np.array([[np.broadcast_to(np.asarray(traj[t][s], dtype=np.float64), (N,)) for t in range(len(c["tp"]))]
                     for s in range(3)])


def cpep_stacked(c, ystar):
    """The case whose B * N subjects are the replicates of c's subjects (replicate-major), observing ystar (B, 1, T, N)."""
    B = ystar.shape[0]
    obs = ystar[:, 0].transpose(0, 2, 1).reshape(-1, ystar.shape[2])
    return dict(c, G=np.tile(c["G"], (B, 1)), obs=obs, age=np.tile(c["age"], B), t2dm=np.tile(c["t2dm"], B))


def supp_evaluator(c, data, scale, n_steps=30, f_info=1.0, f_score=1.0):
    """refine_ref.supp_evaluator on the observations `data` (3, T, M) with the loss weights 1 / scale^2 given."""
    import cude_oracle as o
    import sensitivity_ref as ref

    def ev(x):
        with np.errstate(all="ignore"):
            cx = np.asarray(x, dtype=np.complex128) + 1j * ref.H
            u = ref._stack(o.supp_forward(np, np.asarray(c["nn"], dtype=np.float64), cx, data, c["tp"], c["arch"], n_steps),
                           data.shape[2])
            info, score, sse = ref._summaries(u, data, 1.0 / np.asarray(scale) ** 2)
        return info * f_info, score * f_score, sse
    return ev


def supp_stacked_data(ystar):
    """(B, 3, T, N) -> (3, T, B * N), replicate-major."""
    B, S, T, N = ystar.shape
    return np.ascontiguousarray(ystar.transpose(1, 2, 0, 3).reshape(S, T, B * N))


def refit(ev, center, B, lower, upper, **kw):
    """Rule 4 over the stacked population: dict of (B, N) arrays of refine_ref.refine's outputs."""
    N = np.size(center)
    r = rr.refine(ev, np.tile(np.asarray(center, dtype=np.float64), B), lower, upper, **kw)
    return {k: v.reshape(B, N) for k, v in r.items()}


def summaries(reps, status, ranks):
    """Rule 5: dict(n_used (N,) int32, mean, sd (N,), order (len(ranks), N)) over every subject's non-FAILED replicates in
    replicate order -- a sequential sum, a second pass for the sd, a selection for the ranks."""
    B, N = reps.shape
    ranks = list(ranks)
    n_used = np.zeros(N, dtype=np.int32)
    mean, sd = np.full(N, np.nan), np.full(N, np.nan)
    order = np.full((len(ranks), N), np.nan)
    for i in range(N):
        x = [reps[b, i] for b in range(B) if status[b, i] != rr.FAILED]
        n = len(x)
        n_used[i] = n
        if n == 0:
            continue
        acc = 0.0
        for v in x:
            acc = acc + v
        mean[i] = acc / n
        if n > 1:
            ss = 0.0
            for v in x:
                ss = ss + (v - mean[i]) * (v - mean[i])
            sd[i] = np.sqrt(ss / (n - 1))
        xs = sorted(x)
        for k, r in enumerate(ranks):
            if r < n:
                order[k, i] = xs[r]
    return dict(n_used=n_used, mean=mean, sd=sd, order=order)


# ----------------------------------------------------------------------------- the cases of the two test files
B_DEFAULT, NOISE_SEED = 8, 5


def case(name, B=B_DEFAULT, N=None, yhat=None, center=None, sigma=None):
    """The recipe of tests/test_bootstrap_host.py on a case of tests/test_gpu_refine.py (its populations, boxes and steps):
    centre = the restatement's fit from the case's constant start, sigma = sqrt(SSE / n) there with n = the residual
    rows, noise from np.random.default_rng(5) -- per replicate standard_normal((N, T)) for the c-peptide models and ((3, T,
    N)) for the suppression model.  yhat / center / sigma: taken as given instead (the GPU tests pass the device's own
    prediction, so that both sides fit the same replicate data).  Returns a dict; make_ev(**kw) builds the evaluation of the
    stacked replicate population, kw = refine_ref's f_info / f_score."""
    import test_gpu_refine as tg
    model, arch, n_state, n_def, box, x_const, max_step, space, _ = tg.CASES[name]
    N = n_def if N is None else N
    c = tg._case_data(name, N)
    supp = model == "supp"
    steps = 30 if model != "cpep_sym" else tg.SYM_STEPS
    T = len(c["tp"])
    rows = 3 * T if supp else T
    if supp:
        import cude_oracle as o
        pop, scale = np.asarray(c["data"], dtype=np.float64), o.supp_scale(c["data"])
    else:
        pop, scale = np.asarray(c["obs"], dtype=np.float64).T[None], np.ones(1)
    kw = dict(xtol=1e-7, max_step=max_step)
    if center is None:
        fit = rr.refine(tg._evaluator(name, c)(), np.full(N, x_const), *box, **kw)
        center = fit["x"]
        if sigma is None:
            sigma = np.sqrt(fit["sse"] / rows)
    rng = np.random.default_rng(NOISE_SEED)
    if supp:
        noise = np.stack([rng.standard_normal((3, T, N)).reshape(rows, N) for _ in range(B)])
    else:
        noise = np.stack([rng.standard_normal((N, T)).T for _ in range(B)])
    if yhat is None:
        yhat = supp_yhat(c, center, steps) if supp else cpep_yhat(c, center, steps, n_state, space)
    ystar = replicate_data(yhat, sigma, scale, noise, pop)
    if supp:
        data = supp_stacked_data(ystar)
        make_ev = lambda **k: supp_evaluator(c, data, scale, steps, **k)                       # noqa: E731
    else:
        cs = cpep_stacked(c, ystar)
        make_ev = lambda **k: rr.cpep_evaluator(cs, n_steps=steps, n_state=n_state, cond_space=space, **k)    # noqa: E731
    return dict(c=c, N=N, B=B, T=T, rows=rows, box=box, kw=kw, center=center, sigma=sigma, noise=np.ascontiguousarray(noise),
                yhat=yhat, ystar=ystar, scale=scale, make_ev=make_ev, model=model)


def unstable_pairs(cs):
    """(base refit, mask (B, N) of the pairs whose status or `evals` change under f_info, f_score = 1 +- 1e-9 (together and
    in opposite directions: the study of tests/test_refine_host.py), largest |dx| / (1 + |x|) over the study)."""
    base = refit(cs["make_ev"](), cs["center"], cs["B"], *cs["box"], **cs["kw"])
    bad = np.zeros(base["x"].shape, dtype=bool)
    worst = 0.0
    for f in (1 + 1e-9, 1 - 1e-9):
        for k in (dict(f_info=f, f_score=f), dict(f_info=f, f_score=1.0 / f)):
            r = refit(cs["make_ev"](**k), cs["center"], cs["B"], *cs["box"], **cs["kw"])
            bad |= (r["status"] != base["status"]) | (r["evals"] != base["evals"])
            with np.errstate(invalid="ignore"):
                worst = max(worst, float(np.nanmax(np.abs(r["x"] - base["x"]) / (1 + np.abs(base["x"])))))
    return base, bad, worst
