"""Wall time of the prediction discrepancies and npde per subject: the one-call route (cude_npde) against what the library
offered before it, a host loop of K x (cude_set_params + cude_simulate, whose result is a download) and numpy.

One process, every variant warmed up, the variants alternated inside every repeat, host clock around calls that end in a
synchronisation.  Per model and (subjects N, simulations K):
  (i)   loop: per simulation set_params(None, cond[k]) and simulate(timepoints); then rule 4 and the reduction in numpy
        (batched: moments by einsum, numpy's Cholesky and triangular solves over all subjects at once)
  (ii)  npde on the same host draws (their upload is inside the call)
  (iii) npde on the device's own draws
Before any time is read, (i) and (ii) are compared: the simulated observations must agree in every bit, pd exactly, and npde
wherever numpy's differently rounded factor does not move a rank (the share that differs is printed).

  python tools/time_npde.py [reps] [N:K ...]         (defaults: 5 repeats; 57:1000 10000:64)
  python tools/time_npde.py --only-call N:K          c-peptide, (iii) alone: for a rocprofv3 --kernel-trace --stats run"""
import os
import sys
import time
from statistics import NormalDist

import numpy as np
import torch  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("conditional-ude_amd", "tests", "oracle", ""):
    sys.path.insert(0, os.path.join(ROOT, p))
import bench  # noqa: E402
import npde_ref as nr  # noqa: E402
from conftest import make_supp_case  # noqa: E402
from cude.engine import Engine  # noqa: E402

only_call = "--only-call" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = 5 if only_call or not args or ":" in args[0] else int(args[0])
sizes = [tuple(int(v) for v in a.split(":")) for a in args if ":" in a] or [(57, 1000), (10000, 64)]
INV = np.vectorize(NormalDist().inv_cdf)


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return f"{np.median(ts):10.3f} [{ts.min():10.3f}, {ts.max():10.3f}]"


def cpep_case(N):
    arch = (2, 6, 2)
    nn = bench.glorot(arch, 1234)
    eng, pop = bench.cpep_engine(Engine, arch, 2, N, 777, 0, nn)
    eng.close()
    eng = Engine("cpep", arch, n_steps=30, n_state=2)
    eng.set_population_cpep(pop["tp"], pop["G"], pop["obs"], pop["age"], pop["t2dm"])
    eng.set_params(nn, pop["beta0"])
    return dict(name="c-peptide 2-6-6-1, S = 30", eng=eng, tp=np.asarray(pop["tp"], dtype=np.float64), state=0,
                y_obs=np.ascontiguousarray(np.asarray(pop["obs"], dtype=np.float64).T[1:]), prior=(-0.6, 0.9), sigma=0.05)


def supp_case(N):
    c = make_supp_case(N)
    eng = Engine("supp", c["arch"], n_steps=30)
    eng.set_population_supp(c["tp"], c["data"])
    eng.set_params(c["nn"], np.zeros(N))
    return dict(name="suppression 4-3x5-1, S = 30", eng=eng, tp=c["tp"], state=2, y_obs=np.ascontiguousarray(c["data"][2, 1:]),
                prior=(0.0, 0.5), sigma=0.05)


def numpy_npde(y, y_obs):
    """pd and npde of y (K, R, N) against y_obs (R, N), all subjects at once (every simulation finite)."""
    K = y.shape[0]
    m = y.mean(axis=0)
    d = (y - m).transpose(2, 1, 0)                           # (N, R, K)
    C = d @ d.transpose(0, 2, 1) / (K - 1)
    L = np.linalg.cholesky(C)
    w = np.linalg.solve(L, d)                                # (N, R, K)
    w_obs = np.linalg.solve(L, (y_obs - m).T[:, :, None])    # (N, R, 1)
    lo = 1.0 / (2.0 * K)
    pd = np.clip(np.sum(y < y_obs[None], axis=0) / K, lo, 1.0 - lo)
    below = np.sum(w < w_obs, axis=2).T                      # (R, N)
    return pd, INV(np.clip(below / K, lo, 1.0 - lo)), m, C


def run(case, N, K):
    eng, tp, state = case["eng"], case["tp"], case["state"]
    R = len(tp) - 1
    sigma = np.full(N, case["sigma"])
    pm, ps = case["prior"]
    if only_call:
        for _ in range(3 + reps):
            eng.npde(sigma, K, prior_mean=pm, prior_sd=ps, state=state)
        eng.close()
        return
    scale = 1.0 if state == 0 else float(eng.get_scale()[0][state])
    rng = np.random.default_rng(5)
    cond = pm + ps * rng.standard_normal((K, N))
    noise = rng.standard_normal((K, R, N))
    out = {}

    def loop():
        v = np.empty((K, R, N))
        for k in range(K):
            eng.set_params(None, cond[k])
            v[k] = eng.simulate(tp)[state, 1:, :]
        y = nr.observe(v, sigma, scale, noise)
        out["i"] = (y,) + numpy_npde(y, case["y_obs"])

    def call_host():
        out["ii"] = eng.npde(sigma, K, cond, noise=noise, state=state, want_sims=out.get("want_sims", False))

    def call_device():
        out["iii"] = eng.npde(sigma, K, prior_mean=pm, prior_sd=ps, state=state)
    variants = [("(i)   loop of K set_params + simulate, numpy", loop), ("(ii)  one call, host draws", call_host),
                ("(iii) one call, device draws", call_device)]
    # ---- correctness first
    loop()
    out["want_sims"] = True
    call_host()
    out["want_sims"] = False
    y, pd, npde, m, C = out["i"]
    got = out["ii"]
    same_y = bool(np.array_equal(got["sims"], y))
    same_pd = bool(np.array_equal(got["pd"], pd))
    moved = np.abs(got["npde"] - npde) > 1e-12
    print(f"{case['name']}, N = {N}, K = {K}: sims bit-identical {same_y}, pd equal {same_pd}, npde differs at "
          f"{np.count_nonzero(moved)} of {moved.size} (numpy's factor), status counts {np.bincount(got['status']).tolist()}, "
          f"pooled npde mean {np.nanmean(got['npde']):.3f} var {np.nanvar(got['npde']):.3f}")
    if not (same_y and same_pd and np.count_nonzero(moved) <= 0.01 * moved.size):
        raise SystemExit("the two routes disagree: no time is read")
    times = {k: [] for k, _ in variants}
    for _, f in variants[1:]:
        f()
    for _ in range(reps):
        for k, f in variants:
            t = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t)
    print(f"  {reps} repeats, ms: median [min, max]")
    for k, _ in variants:
        print(f"  {k:46s} {stats(times[k])}")
    print(f"  loop / one call (host draws): {np.median(times[variants[0][0]]) / np.median(times[variants[1][0]]):.1f} x")
    eng.close()


for N, K in sizes:
    run(cpep_case(N), N, K)
    if not only_call:
        run(supp_case(N), N, K)
