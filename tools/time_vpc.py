"""Wall time of the visual predictive check by subject group: the one-call route (cude_vpc) against what the library offered
before it -- cude_npde with sims_out (a download of [K][R][N] doubles) and numpy.quantile over the subjects of every
(simulation, row, group), then over the simulations.

One process, every variant warmed up, the variants alternated inside every repeat, host clock around calls that end in a
synchronisation.  C-peptide model, fixed step, device draws, three groups (subject index mod 3), levels 5 / 50 / 95 %, interval
2.5 / 50 / 97.5 %.  Per (subjects N, simulations K):
  (i)   npde(want_sims=True) on the device's draws, then numpy.quantile per group over subjects and over simulations
  (ii)  vpc on the same draws
Before any time is read the two are compared: observed, simulated quantiles and intervals must agree in every value.

  python tools/time_vpc.py [reps] [N:K ...]          (defaults: 5 repeats; 117:1000 100000:100)
  python tools/time_vpc.py --only-call N:K           (ii) alone: for a rocprofv3 --kernel-trace --stats run"""
import os
import sys
import time

import numpy as np
import torch  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("conditional-ude_amd", "tests", "oracle", ""):
    sys.path.insert(0, os.path.join(ROOT, p))
import bench  # noqa: E402
from cude.engine import Engine  # noqa: E402

only_call = "--only-call" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = 5 if only_call or not args or ":" in args[0] else int(args[0])
sizes = [tuple(int(v) for v in a.split(":")) for a in args if ":" in a] or [(117, 1000), (100000, 100)]
LEVELS, CI, G = (0.05, 0.5, 0.95), (0.025, 0.5, 0.975), 3


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
    eng.set_rng(20251021)
    return eng, np.ascontiguousarray(np.asarray(pop["obs"], dtype=np.float64).T[1:])


def numpy_vpc(sims, y_obs, groups):
    """observed (G, R, L), simulated_q (K, G, R, L), simulated_ci (G, R, L, C) by numpy.quantile (every simulation finite)."""
    obs, sim_q = [], []
    for g in range(G):
        mem = np.flatnonzero(groups == g)
        obs.append(np.quantile(y_obs[:, mem], LEVELS, axis=1).T)                       # (R, L)
        sim_q.append(np.quantile(sims[:, :, mem], LEVELS, axis=2).transpose(1, 2, 0))  # (K, R, L)
    sim_q = np.stack(sim_q, axis=1)
    return np.stack(obs), sim_q, np.moveaxis(np.quantile(sim_q, CI, axis=0), 0, -1)


def run(N, K):
    eng, y_obs = cpep_case(N)
    sigma = np.full(N, 0.05)
    groups = (np.arange(N) % G).astype(np.int32)
    kw = dict(prior_mean=-0.6, prior_sd=0.9)
    if only_call:
        for _ in range(3 + reps):
            eng.vpc(sigma, K, groups=groups, n_groups=G, levels=LEVELS, ci_levels=CI, want_sim_q=False, **kw)
        eng.close()
        return
    out = {}

    def host():
        sims = eng.npde(sigma, K, want_sims=True, want_decorrelated=False, **kw)["sims"]
        out["i"] = numpy_vpc(sims, y_obs, groups)

    def call():
        out["ii"] = eng.vpc(sigma, K, groups=groups, n_groups=G, levels=LEVELS, ci_levels=CI, want_sim_q=out.get("want_q", False),
                            **kw)
    variants = [("(i)   npde sims download + numpy.quantile", host), ("(ii)  one call", call)]
    # ---- correctness first
    host()
    out["want_q"] = True
    call()
    out["want_q"] = False
    obs, sim_q, ci = out["i"]
    got = out["ii"]
    same = [bool(np.array_equal(obs, got["observed"])), bool(np.array_equal(sim_q, got["simulated_q"])),
            bool(np.array_equal(ci, got["simulated_ci"]))]
    print(f"c-peptide 2-6-6-1, S = 30, N = {N}, K = {K}, {G} groups: observed / simulated quantiles / intervals equal {same}; "
          f"members {got['n_members'].tolist()}, simulations used {got['n_sims_used'].tolist()}")
    if not all(same):
        raise SystemExit("the two routes disagree: no time is read")
    times = {k: [] for k, _ in variants}
    call()
    for _ in range(reps):
        for k, f in variants:
            t = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t)
    print(f"  {reps} repeats, ms: median [min, max]")
    for k, _ in variants:
        print(f"  {k:46s} {stats(times[k])}")
    print(f"  download + numpy / one call: {np.median(times[variants[0][0]]) / np.median(times[variants[1][0]]):.1f} x")
    eng.close()


for N, K in sizes:
    run(N, K)
