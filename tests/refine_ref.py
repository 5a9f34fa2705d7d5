"""The iteration of cude_refine_conditional restated in numpy from the rule's text (include/cude.h), over the fixed-step
tangent references of tests/sensitivity_ref.py -- the yardstick the device kernels are held to (tests/test_gpu_refine.py)
and which tests/test_refine_host.py holds against an independent minimiser.

Subject i minimises F(x) = SSE_i(x) + pw (x - pc)^2 over [lower, upper] from x0_i.  An evaluation at x gives
(info, score, sse); g = score + pw (x - pc) is half the gradient, Hgn = info + pw half the Gauss-Newton curvature.

  1. x = clamp(x0); evaluate; lambda = 1e-3; no secant pair.  Non-finite F: FAILED.
  2. c = (g - gp) / (x - xp); H = c if finite and > 0, else Hgn.  Not H > 0: FLAT.
  3. d = clamp(-g / (H (1 + lambda)), +-max_step); xt = clamp(x + d).
  4. |xt - x| <= xtol (1 + |x|): AT_BOUND if xt is a bound, else CONVERGED.
  5. evaluate at xt; accept iff F(xt) finite and < F: (xp, gp) <- (x, g), move, lambda <- max(lambda / 10, 1e-12);
     reject: (xp, gp) <- (xt, g(xt)) if F(xt) was finite, lambda <- 10 lambda.
  6. evals == max_evals: MAX_EVALS (also right behind step 1); otherwise back to 2.

All subjects advance together here (one vectorised evaluation per round, stopped subjects masked), which changes nothing
per subject: no quantity crosses subjects."""
import numpy as np

CONVERGED, AT_BOUND, MAX_EVALS, FLAT, FAILED = range(5)
_RUNNING = -1


def refine(ev, x0, lower, upper, max_evals=40, xtol=1e-7, max_step=0.5, pw=0.0, pc=0.0):
    """ev(x (N,)) -> (info, score, sse), each (N,).  Returns dict(x, objective, sse, info, evals, status)."""
    x = np.clip(np.asarray(x0, dtype=np.float64), lower, upper)
    N = x.size
    info, score, sse = (np.array(v, dtype=np.float64) for v in ev(x))
    F = sse + pw * (x - pc) ** 2
    g = score + pw * (x - pc)
    lam = np.full(N, 1e-3)
    xp, gp = np.full(N, np.nan), np.full(N, np.nan)
    evals = np.ones(N, dtype=np.int32)
    status = np.full(N, _RUNNING, dtype=np.int32)
    bad = ~np.isfinite(F)
    status[bad] = FAILED
    F[bad] = np.inf
    while True:
        status[(status == _RUNNING) & (evals >= max_evals)] = MAX_EVALS                    # 6
        run = status == _RUNNING
        if not run.any():
            break
        with np.errstate(all="ignore"):
            c = (g - gp) / (x - xp)                                                         # 2
            H = np.where(np.isfinite(c) & (c > 0), c, info + pw)
            flat = run & ~(H > 0)
            d = np.clip(-g / (H * (1.0 + lam)), -max_step, max_step)                        # 3
        status[flat] = FLAT
        run &= ~flat
        xt = np.clip(x + d, lower, upper)
        small = run & (np.abs(xt - x) <= xtol * (1.0 + np.abs(x)))                          # 4
        status[small] = np.where((xt[small] == lower) | (xt[small] == upper), AT_BOUND, CONVERGED)
        run &= ~small
        if not run.any():
            break
        xe = np.where(run, xt, x)                                                           # 5
        i2, s2, e2 = (np.asarray(v, dtype=np.float64) for v in ev(xe))
        F2 = e2 + pw * (xe - pc) ** 2
        g2 = s2 + pw * (xe - pc)
        fin = run & np.isfinite(F2)
        acc = fin & (F2 < F)
        rej = run & ~acc
        xp = np.where(acc, x, np.where(rej & fin, xe, xp))
        gp = np.where(acc, g, np.where(rej & fin, g2, gp))
        x, F, g = np.where(acc, xe, x), np.where(acc, F2, F), np.where(acc, g2, g)
        info, sse = np.where(acc, i2, info), np.where(acc, e2, sse)
        lam = np.where(acc, np.maximum(lam / 10.0, 1e-12), np.where(rej, lam * 10.0, lam))
        evals = evals + run
    return dict(x=x, objective=F, sse=sse, info=info, evals=evals, status=status)


# ----------------------------------------------------------------------------- evaluations on the CPU oracle
def cpep_evaluator(c, n_steps=30, n_state=2, cond_space="log", nn=None, arch=None, f_info=1.0, f_score=1.0):
    """c: a case of conftest.make_cpep_case.  f_info / f_score scale every info / score (the perturbation study)."""
    import cude_oracle as o
    import sensitivity_ref as ref
    arch = c["arch"] if arch is None else arch
    nn = c["nn"] if nn is None else nn
    pop = o.CPepPopulation(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"], covariate=(arch[0] == 3))

    def ev(x):
        with np.errstate(all="ignore"):
            _, info, score, sse = ref.cpep_sens(nn, x, pop, arch, n_steps, n_state, cond_space)
        return info * f_info, score * f_score, sse
    return ev


def supp_evaluator(c, n_steps=30, f_info=1.0, f_score=1.0):
    import sensitivity_ref as ref

    def ev(x):
        with np.errstate(all="ignore"):
            _, info, score, sse = ref.supp_sens(c["nn"], x, c["data"], c["tp"], c["arch"], n_steps)
        return info * f_info, score * f_score, sse
    return ev


def scan(ev, N, lower, upper, n_grid=41):
    """(grid values, profile (n_grid, N) of the SSE): the coarse scan a refinement starts from."""
    values = np.linspace(lower, upper, n_grid)
    return values, np.stack([ev(np.full(N, v))[2] for v in values])


def unique_interior_basin(profile, i):
    """Selection of tests/test_gpu_fit.py::test_fit_and_profile_against_the_oracle: the grid argmin of subject i when it
    is interior and no grid point outside its neighbourhood is as deep (within 1e-3), else None."""
    n = profile.shape[0]
    k = int(np.argmin(profile[:, i]))
    others = np.delete(profile[:, i], [max(k - 1, 0), k, min(k + 1, n - 1)])
    if k in (0, n - 1) or others.min() < profile[k, i] * (1 + 1e-3) + 1e-9:
        return None
    return k
