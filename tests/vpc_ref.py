"""cude_vpc's rules 2 ... 6 restated in numpy from the header's text (include/cude.h) -- the yardstick of
tests/test_gpu_vpc.py, which tests/test_vpc_host.py holds against numpy.quantile.  The simulation (rule 1) is cude_npde's:
the cases, host draws, CPU solves and rule 4 are tests/npde_ref.py's, imported here.

Layouts: simulated observations y (K, R, N), observations y_obs (R, N), groups (N,) int; observed (G, R, L), simulated_q (K,
G, R, L), simulated_ci (G, R, L, C).

Rule 3 is written with numpy.sort and scalar arithmetic, one operation per statement: the order statistics are values of
the column, and (n - 1) q, its floor, the difference, the product and the last sum or difference are each rounded once."""
import numpy as np

from npde_ref import case, draws, make_engine, observe, solve_sets  # noqa: F401  (the tests take them from here)

NO_GROUP, FAILED_SIMS, BAD_OBS = 1, 2, 4


def quantile(x, q):
    """Rule 3: the type-7 quantile at level q of the values x (n >= 1 of them)."""
    xs = np.sort(np.asarray(x, dtype=np.float64).reshape(-1))
    n = xs.size
    h = np.float64(n - 1) * np.float64(q)
    fl = np.floor(h)
    lo = int(fl)
    hi = min(lo + 1, n - 1)
    g = h - fl
    x_lo, x_hi = xs[lo], xs[hi]
    d = x_hi - x_lo
    if g >= 0.5:
        w = np.float64(1.0) - g
        p = d * w
        return x_hi - p
    p = d * g
    return x_lo + p


def membership(y_obs, sigma, groups, n_groups):
    """Rule 2: (grp (N,) -- the group a subject counts in, -1 for none --, status (N,) with NO_GROUP / BAD_OBS)."""
    y_obs = np.asarray(y_obs, dtype=np.float64)
    N = y_obs.shape[1]
    ids = np.zeros(N, dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    assert np.all(ids < n_groups)
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (N,))
    bad = ~(np.all(np.isfinite(y_obs), axis=0) & np.isfinite(sigma))
    status = np.where(ids < 0, NO_GROUP, np.where(bad, BAD_OBS, 0)).astype(np.int32)
    return np.where(status != 0, -1, ids), status


def intervals(sim_q, sim_bad, n_members, ci_levels):
    """Rule 6 on simulated quantiles sim_q (K, G, R, L) with the left-out simulations sim_bad (K, G): (G, R, L, C)."""
    K, G, R, L = sim_q.shape
    out = np.full((G, R, L, len(ci_levels)), np.nan)
    for g in range(G):
        use = ~sim_bad[:, g]
        if n_members[g] == 0 or not use.any():
            continue
        for r in range(R):
            for l in range(L):
                for c, q in enumerate(ci_levels):
                    out[g, r, l, c] = quantile(sim_q[use, g, r, l], q)
    return out


def vpc(y, y_obs, sigma, groups, n_groups, levels, ci_levels, sim_q=None):
    """Rules 2 ... 6: dict(observed, simulated_q, simulated_ci, n_members, n_sims_used, status, outside).  sim_q: take rule 6
    over these simulated quantiles (the device's own) instead of the restated ones."""
    y = np.asarray(y, dtype=np.float64)
    y_obs = np.asarray(y_obs, dtype=np.float64)
    K, R, N = y.shape
    G, L = int(n_groups), len(levels)
    grp, status = membership(y_obs, sigma, groups, G)
    finite = np.all(np.isfinite(y), axis=1)                                   # (K, N)
    observed = np.full((G, R, L), np.nan)
    q_sim = np.full((K, G, R, L), np.nan)
    sim_bad = np.zeros((K, G), dtype=bool)
    n_members = np.zeros(G, dtype=np.int32)
    for g in range(G):
        mem = np.flatnonzero(grp == g)
        n_members[g] = mem.size
        if mem.size == 0:
            continue
        sim_bad[:, g] = ~np.all(finite[:, mem], axis=1)
        status[mem[np.any(~finite[:, mem], axis=0)]] |= FAILED_SIMS
        for r in range(R):
            for l, q in enumerate(levels):
                observed[g, r, l] = quantile(y_obs[r, mem], q)
                for k in np.flatnonzero(~sim_bad[:, g]):
                    q_sim[k, g, r, l] = quantile(y[k, r, mem], q)
    ci = intervals(q_sim if sim_q is None else np.asarray(sim_q), sim_bad, n_members, ci_levels)
    with np.errstate(invalid="ignore"):
        outside = (observed < ci[..., 0]) | (observed > ci[..., -1])
    return dict(observed=observed, simulated_q=q_sim, simulated_ci=ci, n_members=n_members,
                n_sims_used=(K - sim_bad.sum(axis=0)).astype(np.int32), status=status, outside=outside)


def same(a, b):
    """Values equal, NaNs matched by position."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=(a.dtype.kind == "f"))


# ----------------------------------------------------------------------------- the calibration study (tests/test_vpc_host.py)
K_CAL, N_CAL = 200, 67
CAL_DATA_SEED = 3          # chosen on the CPU (tests/test_vpc_host.py): the restatement alone shows 0 of 15 cells outside
CAL_LEVELS, CAL_CI = (0.05, 0.5, 0.95), (0.025, 0.5, 0.975)


def calibration(data_seed, obs_shift=0.0):
    """A well-specified case: cpep-2441 with N_CAL subjects whose data are draws from the model (seed data_seed, the random
    effects' mean shifted by obs_shift prior_sd), K_CAL simulations from host draws on the CPU oracle, one group.  Returns
    (case, cond_sets, noise, y, restated outputs)."""
    cs = case("cpep-2441", N_CAL, data_seed=data_seed, obs_shift=obs_shift)
    cond, noise = draws(cs, K_CAL, seed=29)
    y = observe(solve_sets(cs, cond), cs["sigma"], cs["scale"], noise)
    return cs, cond, noise, y, vpc(y, cs["y_obs"], cs["sigma"], None, 1, CAL_LEVELS, CAL_CI)
