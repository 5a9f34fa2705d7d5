"""cude_npde restated in numpy from the rules' text (include/cude.h): the draws of rules 2 and 4 (Philox counters of the two
block kinds of csrc/cude_rng.h), the simulated observations of rule 4, the used simulations, moments, pd, Cholesky
decorrelation and npde of rules 5 ... 9, with Wichura's AS241 (PPND16) written out -- the yardstick of
tests/test_gpu_npde.py, which tests/test_npde_host.py holds against numpy's own statistics and admits case by case.

Layouts: simulated observations y (K, R, N), observations y_obs (R, N), R = T - 1 rows t_1 ... t_{T-1}; conditional sets
(K, N); noise (K, R, N).

Every floating-point sum of the rules is sequential in k per entry; here the loop over k is a Python loop and every step a
numpy operation over all entries at once -- each product and each sum rounded on its own, as the rules say."""
import functools
import math

import numpy as np

SINGULAR, FEW, FAILED_SIMS, BAD_OBS = 1, 2, 4, 8
KIND_ETA, KIND_NOISE = 0x80008000, 0x80004000
PIVOT_TOL = 2.0 ** -40
EPS = 2.0 ** -52


# ----------------------------------------------------------------------------- AS241
_A = (3.3871328727963666080e0, 1.3314166789178437745e2, 1.9715909503065514427e3, 1.3731693765509461125e4,
      4.5921953931549871457e4, 6.7265770927008700853e4, 3.3430575583588128105e4, 2.5090809287301226727e3)
_B = (1.0, 4.2313330701600911252e1, 6.8718700749205790830e2, 5.3941960214247511077e3, 2.1213794301586595867e4,
      3.9307895800092710610e4, 2.8729085735721942674e4, 5.2264952788528545610e3)
_C = (1.42343711074968357734e0, 4.63033784615654529590e0, 5.76949722146069140550e0, 3.64784832476320460504e0,
      1.27045825245236838258e0, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4)
_D = (1.0, 2.05319162663775882187e0, 1.67638483018380384940e0, 6.89767334985100004550e-1, 1.48103976427480074590e-1,
      1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9)
_E = (6.65790464350110377720e0, 5.46378491116411436990e0, 1.78482653991729133580e0, 2.96560571828504891230e-1,
      2.65321895265761230930e-2, 1.24266094738807843860e-3, 2.71155556874348757815e-5, 2.01033439929228813265e-7)
_F = (1.0, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2, 7.86869131145613259100e-4,
      1.84631831751005468180e-5, 1.42151175831644588870e-7, 2.04426310338993978564e-15)


def _horner(c, r):
    acc = c[7]
    for v in c[6::-1]:
        acc = acc * r + v
    return acc


def as241(p):
    """Wichura (1988), Algorithm AS241, PPND16: the standard normal quantile of p in (0, 1)."""
    q = p - 0.5
    if abs(q) <= 0.425:
        r = 0.180625 - q * q
        return _horner(_A, r) * q / _horner(_B, r)
    r = math.sqrt(-math.log(p if q < 0.0 else 1.0 - p))
    if r <= 5.0:
        r = r - 1.6
        x = _horner(_C, r) / _horner(_D, r)
    else:
        r = r - 5.0
        x = _horner(_E, r) / _horner(_F, r)
    return -x if q < 0.0 else x


def clipped(count, n):
    """Rules 7 and 8: count / n clipped to [1 / (2 n), 1 - 1 / (2 n)]."""
    lo = 1.0 / (2.0 * n)
    hi = 1.0 - lo
    return min(max(count / n, lo), hi)


# ----------------------------------------------------------------------------- draws
def _u01(hi, lo):
    return ((((hi << 32) | lo) >> 11) + 0.5) * 2.0 ** -53


def counter(subject, rep, kind_row):
    """The Philox counter of a draw of (global subject, replicate) in block kind | row `kind_row` (csrc/cude_rng.h)."""
    return [subject & 0xFFFFFFFF, (subject >> 32) & 0xFFFFFFFF, rep & 0xFFFFFFFF, kind_row | (((rep >> 32) & 0x7FFF) << 16)]


def _normal(seed, ctr):
    from conftest import philox4x32_10
    c = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return math.sqrt(-2.0 * math.log(_u01(c[0], c[1]))) * math.cos(2.0 * math.pi * _u01(c[2], c[3]))


def eta_normal(seed, subject, rep):
    """Rule 2's z of (seed, global subject, replicate) (Box-Muller through libm here: a few ulp from the device's)."""
    return _normal(seed, counter(subject, rep, KIND_ETA))


def noise_normal(seed, subject, rep, row):
    """Rule 4's eps of (seed, global subject, replicate, row)."""
    return _normal(seed, counter(subject, rep, KIND_NOISE | row))


# ----------------------------------------------------------------------------- rules 4 ... 9
def observe(v, sigma, scale, eps):
    """Rule 4: v + (sigma s) eps, every operation rounded on its own.  v, eps (K, R, N); sigma (N,)."""
    amp = np.asarray(sigma, dtype=np.float64) * float(scale)
    d = amp[None, None, :] * eps
    return v + d


def reduce(y, y_obs, sigma, want_aux=False):
    """Rules 5 ... 9 on simulated observations y (K, R, N) against y_obs (R, N): dict(pred_mean, pred_var, pd, npde (R, N),
    below, below_decorr (R, N) int32, n_used, status (N,) int32).  want_aux: also w (K, R, N), w_obs (R, N), cov (R, R, N) and
    used (K, N) -- what the admission of a case looks at."""
    y = np.asarray(y, dtype=np.float64)
    K, R, N = y.shape
    with np.errstate(all="ignore"):
        used = np.all(np.isfinite(y), axis=1)                            # (K, N)
        bad = ~(np.all(np.isfinite(y_obs), axis=0) & np.isfinite(sigma))
        n = used.sum(axis=0).astype(np.int64)
        acc = np.zeros((R, N))
        below = np.zeros((R, N), dtype=np.int64)
        for k in range(K):
            acc = np.where(used[k], acc + y[k], acc)
            below += used[k] & (y[k] < y_obs)
        m = acc / n
        cov = np.zeros((R, R, N))
        for k in range(K):
            d = y[k] - m
            q = d[:, None, :] * d[None, :, :]
            cov = np.where(used[k], cov + q, cov)
        cov = cov / (n - 1)
        status = np.where(bad, BAD_OBS, 0).astype(np.int32)
        status[~bad & (n < K)] |= FAILED_SIMS
        few = ~bad & (n <= R)
        status[few] |= FEW
        L = np.zeros((R, R, N))
        singular = np.zeros(N, dtype=bool)
        for r in range(R):
            for s in range(r):
                a = cov[r, s].copy()
                for j in range(s):
                    a = a - L[r, j] * L[s, j]
                L[r, s] = a / L[s, s]
            p = cov[r, r].copy()
            for j in range(r):
                p = p - L[r, j] * L[r, j]
            singular |= ~(p > PIVOT_TOL * cov[r, r])
            L[r, r] = np.sqrt(p)
        status[~bad & ~few & singular] |= SINGULAR

        def solve(rhs):                                                  # rhs (..., R, N) -> w
            w = np.zeros_like(rhs)
            for r in range(R):
                a = rhs[..., r, :] - m[r]
                for j in range(r):
                    a = a - L[r, j] * w[..., j, :]
                w[..., r, :] = a / L[r, r]
            return w
        w_obs, w = solve(np.asarray(y_obs, dtype=np.float64)), solve(y)
        below_d = np.sum(used[:, None, :] & (w < w_obs[None]), axis=0)
    none = (status & (SINGULAR | FEW | BAD_OBS)) != 0
    pd, npde = np.full((R, N), np.nan), np.full((R, N), np.nan)
    for i in range(N):
        if bad[i]:
            continue
        for r in range(R):
            if n[i] > 0:
                pd[r, i] = clipped(int(below[r, i]), int(n[i]))
            if not none[i]:
                npde[r, i] = as241(clipped(int(below_d[r, i]), int(n[i])))
    out = dict(pred_mean=np.where(bad, np.nan, m), pred_var=np.where(bad, np.nan, cov[np.arange(R), np.arange(R)]), pd=pd,
               npde=npde, below=np.where(bad, -1, below).astype(np.int32),
               below_decorr=np.where(none, -1, below_d).astype(np.int32), n_used=np.where(bad, -1, n).astype(np.int32),
               status=status)
    if want_aux:
        out.update(w=w, w_obs=w_obs, cov=cov, used=used)
    return out


def near_ties(aux):
    """The admission rule: pair (r, i) is a near-tie when min_k |w_kr - w_obs_r| < 16 R^2 eps cond(C_i) (1 + |w_obs_r|).
    Returns (mask (R, N), cond (N,)) over the subjects with a decorrelation (elsewhere False / NaN)."""
    w, w_obs, cov, used = aux["w"], aux["w_obs"], aux["cov"], aux["used"]
    K, R, N = w.shape
    ok = (aux["status"] & (SINGULAR | FEW | BAD_OBS)) == 0
    cond = np.full(N, np.nan)
    mask = np.zeros((R, N), dtype=bool)
    for i in np.flatnonzero(ok):
        cond[i] = np.linalg.cond(cov[:, :, i])
        margin = np.min(np.abs(w[used[:, i], :, i] - w_obs[None, :, i]), axis=0)
        mask[:, i] = margin < 16.0 * R * R * EPS * cond[i] * (1.0 + np.abs(w_obs[:, i]))
    return mask, cond


def pooled(npde):
    """Mean and unbiased variance of the finite entries."""
    x = npde[np.isfinite(npde)]
    return float(np.mean(x)), float(np.var(x, ddof=1))


# ----------------------------------------------------------------------------- the cases of the two test files
N_CASE, T_CASE = 70, 6
# name -> (model, arch, n_state, n_steps, cond_space, state, prior_mean, prior_sd, seed of the population)
CASES = {
    "cpep-2441": ("cpep", (2, 4, 2), 2, 12, "log", 0, -0.6, 0.5, 20250905),
    "cpep-3441": ("cpep", (3, 4, 2), 3, 18, "log", 0, -0.6, 0.5, 11),
    "supp-4355": ("supp", (4, 3, 5), 3, 30, "log", 2, 0.0, 0.5, 7),
    "sym-raw": ("cpep_sym", (1, 0, 0), 2, 24, "raw", 0, 20.0, 3.0, 20250905),
}
SYM_P0 = 1.78


def _cpep_population(N, seed, T):
    """conftest.make_cpep_case's synthetic subjects on T equidistant times: the glucose curves interpolated linearly."""
    import cude_oracle as o
    tp5, G5, cp, age, t2, beta_true, rng = o.synthetic_cpep_population(N, seed)
    tp = np.linspace(0.0, 120.0, T)
    G = np.stack([np.interp(tp, tp5, G5[i]) for i in range(N)])
    return tp, G, np.repeat(cp[:, :1], T, axis=1), age, t2


def _supp_population(N, seed, T):
    """conftest.make_supp_case's curves on T times over [0, 30]."""
    rng = np.random.default_rng(seed)
    tp = np.linspace(0.0, 30.0, T)
    t = tp[None, :, None]
    k = 0.3 + 0.2 * rng.random((1, 1, N))
    data = np.empty((3, T, N))
    data[0] = (10.0 * np.exp(-0.4 * t))[0]
    data[1] = (6.0 * t * np.exp(-k * t) / 3.0)[0] + 0.2
    data[2] = (4.0 * (1 - np.exp(-0.15 * t)) * np.exp(-0.02 * t))[0] + 0.1
    data = np.maximum(data * (1.0 + 0.1 * rng.standard_normal(data.shape)), 0.0)
    data[0, 0] = 10.0 * (1 + 0.05 * rng.standard_normal(N))
    return tp, data


def solve_sets(cs, cond_sets):
    """Rule 3 on the CPU oracle: v (K, R, N) of the case's state at t_1 ... for conditional sets (K, N) -- the K * N
    (set, subject) pairs solved as one stacked population."""
    import cude_oracle as o
    cond_sets = np.asarray(cond_sets, dtype=np.float64)
    K, N = cond_sets.shape
    T = len(cs["tp"])
    with np.errstate(all="ignore"):
        if cs["model"] == "supp":
            traj = o.supp_forward(np, cs["nn"], cond_sets.reshape(-1), np.tile(cs["data"], (1, 1, K)), cs["tp"], cs["arch"],
                                  cs["n_steps"])
        else:
            pop = o.CPepPopulation(cs["tp"], np.tile(cs["G"], (K, 1)), np.tile(cs["obs"], (K, 1)), np.tile(cs["age"], K),
                                   np.tile(cs["t2dm"], K), covariate=(cs["arch"][0] == 3))
            traj = o.cpep_forward(np, cs["nn"], cond_sets.reshape(-1), pop, cs["arch"], cs["n_steps"], cs["n_state"],
                                  cs["cond_space"])
    s = cs["state"]
    v = np.stack([np.broadcast_to(np.asarray(traj[t][s], dtype=np.float64), (K * N,)) for t in range(1, T)])      # (R, K N)
    return np.ascontiguousarray(v.reshape(T - 1, K, N).transpose(1, 0, 2))


@functools.lru_cache(maxsize=None)
def case(name, N=N_CASE, T=T_CASE, data_seed=3, obs_shift=0.0):
    """A population of N subjects on T times whose observations are drawn from the model itself: eta_i ~ Normal(prior_mean
    + obs_shift prior_sd, prior_sd), the oracle's solve, residual noise of standard deviation sigma_i times the state's scale
    (draws of np.random.default_rng(data_seed)).  Returns a dict (treat it as read-only: it is shared between tests)."""
    import cude_oracle as o
    model, arch, n_state, n_steps, space, state, pm, ps, seed = CASES[name]
    cs = dict(name=name, model=model, arch=arch, n_state=n_state, n_steps=n_steps, cond_space=space, state=state,
              prior_mean=pm, prior_sd=ps, N=N, T=T, R=T - 1)
    rng = np.random.default_rng(data_seed)
    eta = pm + obs_shift * ps + ps * rng.standard_normal(N)
    eps = rng.standard_normal((1, T - 1, N))
    if model == "supp":
        tp, data = _supp_population(N, seed, T)
        cs.update(tp=tp, data=data, nn=o.glorot_params(arch, seed + 1))
        cs["scale"] = float(o.supp_scale(data)[state])
        cs["sigma"] = 0.04 + 0.01 * (np.arange(N) % 3)
    else:
        tp, G, obs, age, t2 = _cpep_population(N, seed, T)
        nn = np.array([SYM_P0]) if model == "cpep_sym" else o.glorot_params(arch, seed + 1)
        cs.update(tp=tp, G=G, obs=obs, age=age, t2dm=t2, nn=nn, scale=1.0)
        cs["sigma"] = 0.03 + 0.01 * (np.arange(N) % 3)
    y = observe(solve_sets(cs, eta[None]), cs["sigma"], cs["scale"], eps)[0]      # (R, N)
    if model == "supp":
        cs["data"] = cs["data"].copy()
        cs["data"][state, 1:, :] = y
        cs["scale"] = float(o.supp_scale(cs["data"])[state])       # (the loss scale is the data's own: cude_get_scale's)
    else:
        cs["obs"] = cs["obs"].copy()
        cs["obs"][:, 1:] = y.T
    cs["y_obs"] = y
    cs["eta_true"] = eta
    return cs


def draws(cs, K, seed=17):
    """Host draws of a case: (cond_sets (K, N) by rule 2's expression from standard normals, noise (K, R, N))."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((K, cs["N"]))
    d = cs["prior_sd"] * z
    return cs["prior_mean"] + d, rng.standard_normal((K, cs["R"], cs["N"]))


def make_engine(cs, n_steps=None, options=(), subjects=None, subject_offset=0):
    """The device context of a case with the shared parameters set (subjects: a slice of the population)."""
    from cude.engine import Engine
    sl = slice(None) if subjects is None else subjects
    steps = cs["n_steps"] if n_steps is None else n_steps
    if cs["model"] == "supp":
        eng = Engine("supp", cs["arch"], n_steps=steps)
        for k, v in options:
            eng.set_option(k, v)
        eng.set_population_supp(cs["tp"], np.ascontiguousarray(cs["data"][:, :, sl]))
    else:
        eng = Engine(cs["model"], cs["arch"], n_steps=steps, n_state=cs["n_state"], cond_space=cs["cond_space"])
        for k, v in options:
            eng.set_option(k, v)
        eng.set_population_cpep(cs["tp"], cs["G"][sl], cs["obs"][sl], cs["age"][sl], cs["t2dm"][sl])
    eng.set_params(cs["nn"], None)
    return eng


K_CAL = 500


@functools.lru_cache(maxsize=None)
def calibration(shift=0.0):
    """The calibration study of tests/test_npde_host.py: the cpep-2441 case (its data are draws from the model), K_CAL
    simulations from host draws of seed 23 with prior_mean shifted by `shift` prior_sd, on the CPU oracle.  Returns (case,
    cond_sets, noise, restated outputs with aux)."""
    cs = case("cpep-2441")
    rng = np.random.default_rng(23)
    z = rng.standard_normal((K_CAL, cs["N"]))
    pm = cs["prior_mean"] + shift * cs["prior_sd"]
    cond = pm + cs["prior_sd"] * z
    noise = rng.standard_normal((K_CAL, cs["R"], cs["N"]))
    y = observe(solve_sets(cs, cond), cs["sigma"], cs["scale"], noise)
    return cs, cond, noise, reduce(y, cs["y_obs"], cs["sigma"], want_aux=True)
