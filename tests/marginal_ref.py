"""Rules 1-4 of cude_marginal_likelihood (include/cude.h) restated in mpmath at 50 digits, fed by given points, SSEs and
node terms: whatever produced the SSEs (the device's own solves in the GPU tests, a closed form in the host tests), the
marginal likelihood and the posterior moments that follow from them are these numbers.

Rule 3's running maximum and rescaling are an evaluation order, not a different value: the sums of exp(t - M) do not
depend on which M the terms are referred to, so the restatement takes M = max t and sums once."""
import mpmath as mp
import numpy as np

mp.mp.dps = 50


def log_weights_of_draws(z):
    """rule 1, device draws: a = c_K + z^2 / 2 with c_K = log(2 pi) / 2 - log K, as mp numbers (K, N)"""
    K = len(z)
    c_K = mp.log(2 * mp.pi) / 2 - mp.log(K)
    return [[c_K + mp.mpf(float(v)) ** 2 / 2 for v in row] for row in z]


def term(a, x, sse, n_obs, sigma, prior_mean, prior_sd):
    """rule 2 for one node: t = a + ll + lp as an mp number, or None for a bad node (non-finite SSE or term)"""
    if not np.isfinite(sse) or (np.isfinite(prior_sd) and not np.isfinite(x)):
        return None
    s2 = mp.mpf(float(sigma)) ** 2
    ll = -mp.mpf(n_obs) / 2 * mp.log(s2) - mp.mpf(float(sse)) / (2 * s2)
    lp = mp.mpf(0)
    if np.isfinite(prior_sd):
        sd = mp.mpf(float(prior_sd))
        lp = -((mp.mpf(float(x)) - mp.mpf(float(prior_mean))) / sd) ** 2 / 2 - mp.log(sd) - mp.log(2 * mp.pi) / 2
    t = (a if isinstance(a, mp.mpf) else mp.mpf(float(a))) + ll + lp
    return t if abs(t) < mp.mpf(2) ** 1024 else None


def marginal(z, a, x, sse, center, scale, n_obs, sigma, prior_mean, prior_sd):
    """z, x, sse: (K, N) doubles (z (K,) for a shared rule); a: (K,) doubles, (K, N) doubles or mp numbers (None: the
    draws' log_weights_of_draws(z)); center, scale: (N,).  Returns a dict of (N,) arrays: logml, post_mean, post_var,
    post_sse, ess (doubles rounded from the mp values), n_bad (int32), terms (K, N) doubles (-Inf = bad), and the
    magnitudes the error bars are made of: tmax = max_k |t| over the good nodes, zmax = max_k |z|, second = scale^2 S2 / S0."""
    x, sse = np.asarray(x, dtype=np.float64), np.asarray(sse, dtype=np.float64)
    K, N = x.shape
    z = np.asarray(z, dtype=np.float64)
    z = np.broadcast_to(z[:, None], (K, N)) if z.ndim == 1 else z
    if a is None:
        a = log_weights_of_draws(z)
    elif isinstance(a, np.ndarray) and a.ndim == 1:
        a = np.broadcast_to(a[:, None], (K, N))
    out = {k: np.full(N, np.nan) for k in ("post_mean", "post_var", "post_sse", "ess", "tmax", "zmax", "second")}
    out["logml"] = np.full(N, -np.inf)
    out["n_bad"] = np.zeros(N, dtype=np.int32)
    out["terms"] = np.full((K, N), -np.inf)
    for i in range(N):
        c, s = float(center[i]), float(scale[i])
        ok = np.isfinite(c) and np.isfinite(s) and s > 0.0
        t = [term(a[k][i], x[k, i], sse[k, i], n_obs, sigma, prior_mean, prior_sd) if ok else None for k in range(K)]
        good = [k for k in range(K) if t[k] is not None]
        out["n_bad"][i] = K - len(good)
        for k in good:
            out["terms"][k, i] = float(t[k])
        if not good:
            continue
        M = max(t[k] for k in good)
        e = {k: mp.exp(t[k] - M) for k in good}
        zk = {k: mp.mpf(float(z[k, i])) for k in good}
        S0 = mp.fsum(e.values())
        S1 = mp.fsum(e[k] * zk[k] for k in good)
        S2 = mp.fsum(e[k] * zk[k] ** 2 for k in good)
        S3 = mp.fsum(e[k] * mp.mpf(float(sse[k, i])) for k in good)
        Q = mp.fsum(e[k] ** 2 for k in good)
        cs, ss = mp.mpf(c), mp.mpf(s)
        out["logml"][i] = float(M + mp.log(S0) + mp.log(ss))
        out["post_mean"][i] = float(cs + ss * S1 / S0)
        out["post_var"][i] = float(ss ** 2 * max(mp.mpf(0), S2 / S0 - (S1 / S0) ** 2))
        out["post_sse"][i] = float(S3 / S0)
        out["ess"][i] = float(S0 ** 2 / Q)
        out["tmax"][i] = max(abs(float(t[k])) for k in good)
        out["zmax"][i] = float(np.max(np.abs(z[:, i])))
        out["second"][i] = float(ss ** 2 * S2 / S0)
    return out


def gaussian_case(c, h, xhat, n_obs, sigma, prior_mean, prior_sd):
    """SSE(x) = c + h (x - xhat)^2 with a Normal(prior_mean, prior_sd) prior: the exponent is a quadratic in x, so the
    integral is Gaussian in closed form.  Returns (logml, mode, sd of the posterior, E[SSE]) as mp numbers."""
    c, h, xhat, sigma, pm, sd = (mp.mpf(float(v)) for v in (c, h, xhat, sigma, prior_mean, prior_sd))
    s2 = sigma ** 2
    A = h / (2 * s2) + 1 / (2 * sd ** 2)                        # exponent = K0 - A (x - m)^2
    m = (h / (2 * s2) * xhat + pm / (2 * sd ** 2)) / A
    at_mode = (-mp.mpf(n_obs) / 2 * mp.log(s2) - (c + h * (m - xhat) ** 2) / (2 * s2)
               - ((m - pm) / sd) ** 2 / 2 - mp.log(sd) - mp.log(2 * mp.pi) / 2)
    var = 1 / (2 * A)
    return at_mode + mp.log(mp.pi / A) / 2, m, mp.sqrt(var), c + h * ((m - xhat) ** 2 + var)


# ---- the same integrals from the numpy oracle's solves (oracle/cude_oracle.py, cpep_loss): what the end-to-end GPU test
# holds the device's two routes to, and how far the routes differ on the oracle itself
def oracle_sse(c, x, n_steps=30):
    """SSE of every subject of the c-peptide case c at every row of x (K, N): one vectorised oracle solve of K N subjects"""
    import cude_oracle as o
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    K, N = x.shape
    tile = lambda v: np.tile(np.asarray(v), (K,) + (1,) * (np.ndim(v) - 1))
    pop = o.CPepPopulation(c["tp"], tile(c["G"]), tile(c["obs"]), tile(c["age"]), tile(c["t2dm"]))
    return o.cpep_loss(np, c["nn"], x.reshape(-1), pop, c["arch"], n_steps)[1].reshape(K, N)


def oracle_laplace(c, sigma, prior_mean, omega, lower=-6.0, upper=4.0, n_grid=81, n_steps=30):
    """(MAP, Laplace scale sigma / sqrt(info + (sigma / omega)^2)) of every subject: the 81-point scan, 60 golden-section
    steps inside the bracket around its argmin, info = sum_j (d yhat_j / d beta)^2 by central differences (h = 1e-5)"""
    import cude_oracle as o
    pw = (sigma / omega) ** 2
    N = len(c["beta"])
    F = lambda x: oracle_sse(c, x, n_steps) + pw * (np.atleast_2d(x) - prior_mean) ** 2
    grid = np.linspace(lower, upper, n_grid)
    k = np.argmin(F(np.repeat(grid[:, None], N, axis=1)), axis=0)
    a, b = grid[np.maximum(k - 1, 0)], grid[np.minimum(k + 1, n_grid - 1)]
    g = (np.sqrt(5.0) - 1.0) / 2.0
    for _ in range(60):
        x1, x2 = b - g * (b - a), a + g * (b - a)
        left = F(x1)[0] < F(x2)[0]
        a, b = np.where(left, a, x1), np.where(left, x2, b)
    m = 0.5 * (a + b)
    pop = o.CPepPopulation(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
    y = lambda x: np.stack([t[0] for t in o.cpep_forward(np, c["nn"], x, pop, c["arch"], n_steps)])
    h = 1e-5
    info = np.sum(((y(m + h) - y(m - h)) / (2 * h)) ** 2, axis=0)
    return m, sigma / np.sqrt(info + pw)


def oracle_logml(c, z, a, center, scale, sigma, prior_mean, omega, n_steps=30):
    """`marginal` on the oracle's SSEs at x = center + scale z"""
    x = center[None, :] + scale[None, :] * np.asarray(z)[:, None]
    return marginal(z, np.asarray(a), x, oracle_sse(c, x, n_steps), center, scale, len(c["tp"]), sigma, prior_mean, omega)


def marginal_numpy(z, a, x, sse, center, scale, n_obs, sigma, prior_mean, prior_sd):
    """The same in doubles (a log-sum-exp about the largest term; all nodes good): for sums of thousands of nodes whose
    result is needed to 1e-12 only.  z, a: (K,) or (K, N).  Returns dict(logml, ess)."""
    z, a = (np.broadcast_to(v[:, None], x.shape) if np.ndim(v) == 1 else np.asarray(v) for v in (np.asarray(z), np.asarray(a)))
    t = a - (n_obs / 2) * np.log(sigma ** 2) - sse / (2 * sigma ** 2)
    t = t - 0.5 * ((x - prior_mean) / prior_sd) ** 2 - np.log(prior_sd) - 0.5 * np.log(2 * np.pi)
    M = t.max(axis=0)
    e = np.exp(t - M)
    S0 = e.sum(axis=0)
    return {"logml": M + np.log(S0) + np.log(scale), "ess": S0 ** 2 / (e * e).sum(axis=0)}


# the end-to-end case of tests/test_gpu_marginal.py: cpep-2441, six subjects, 30 steps
E2E = dict(N=6, arch=(2, 4, 2), n_steps=30, sigma=0.03, prior_mean=-1.0, omega=0.8, halfwidth=8.0, n_grid=4001, seed=20250905,
           n_draws=2048)
_E2E_ORACLE = {}


def end_to_end_oracle():
    """Both rules on the numpy oracle for exactly that case, computed once: dict(case, grid, q33, q1 (N,) logml, keep (N,)
    bool = subjects whose 33-node rule and grid agree to 1e-6, center, scale)."""
    if not _E2E_ORACLE:
        from conftest import make_cpep_case
        from cude import api
        e = E2E
        c = make_cpep_case(e["N"], e["arch"])
        N, T = e["N"], len(c["tp"])
        m, s = oracle_laplace(c, e["sigma"], e["prior_mean"], e["omega"], n_steps=e["n_steps"])
        zg, ag = api.grid_rule(e["prior_mean"] - e["halfwidth"] * e["omega"], e["prior_mean"] + e["halfwidth"] * e["omega"],
                               e["n_grid"])
        xg = np.repeat(zg[:, None], N, axis=1)
        grid = marginal_numpy(zg, ag, xg, oracle_sse(c, xg, e["n_steps"]), np.zeros(N), np.ones(N), T, e["sigma"],
                              e["prior_mean"], e["omega"])["logml"]
        out = dict(case=c, grid=grid, center=m, scale=s)
        for Q in (33, 1):
            z, a = api.gauss_hermite_rule(Q)
            x = m[None, :] + s[None, :] * z[:, None]
            out[f"q{Q}"] = marginal_numpy(z, a, x, oracle_sse(c, x, e["n_steps"]), m, s, T, e["sigma"], e["prior_mean"],
                                          e["omega"])["logml"]
        out["keep"] = np.abs(out["q33"] - grid) <= 1e-6
        _E2E_ORACLE.update(out)
    return _E2E_ORACLE
