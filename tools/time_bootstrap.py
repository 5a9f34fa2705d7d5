"""Wall time of the parametric bootstrap of the per-subject fits: the one-launch route (cude_bootstrap_conditional) against
what the library offered before it, a host loop of B x (upload the replicate's observations + cude_refine_conditional).

One process, every variant warmed up, the variants alternated inside every repeat, host clock around calls that end in a
synchronisation.  Per model and (subjects N, replicates B):
  (i)   loop: per replicate set_population_* with the replicate's observations (suppression: + set_global_subjects, so that
        the loss weights stay the population's) and refine_conditional from the centre
  (ii)  bootstrap_conditional on the same host noise (its upload is inside the call)
  (iii) bootstrap_conditional on the device's own draws
Before any time is read, (i) and (ii) are compared: the same replicates must give the same points within the x bar of
tests/test_gpu_refine.py, 1e-6 (1 + |x|), and the same statuses.  Evaluations per replicate fit (mean, max) are the loop's
(the one-launch route reports points and statuses only).

  python tools/time_bootstrap.py [reps] [N:B ...]        (defaults: 5 repeats; 57:256 57:1000 10000:64 100000:16)
  python tools/time_bootstrap.py --only-launch N:B       c-peptide, (iii) alone: for a rocprofv3 --kernel-trace --stats run"""
import os
import sys
import time

import numpy as np
import torch  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("conditional-ude_amd", "tests", "oracle", ""):
    sys.path.insert(0, os.path.join(ROOT, p))
import bench  # noqa: E402
import bootstrap_ref as br  # noqa: E402
from conftest import make_supp_case  # noqa: E402
from cude.engine import Engine  # noqa: E402

only_launch = "--only-launch" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = 5 if only_launch or not args or ":" in args[0] else int(args[0])
sizes = [tuple(int(v) for v in a.split(":")) for a in args if ":" in a] or [(57, 256), (57, 1000), (10000, 64), (100000, 16)]
X_BAR = 1e-6


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return f"{np.median(ts):10.3f} [{ts.min():10.3f}, {ts.max():10.3f}]"


def cpep_case(N):
    arch = (2, 6, 2)
    nn = bench.glorot(arch, 1234)
    eng0, pop = bench.cpep_engine(Engine, arch, 2, N, 777, 0, nn)
    eng0.close()

    def make(obs=None):
        eng = Engine("cpep", arch, n_steps=30, n_state=2)
        eng.set_population_cpep(pop["tp"], pop["G"], pop["obs"] if obs is None else obs, pop["age"], pop["t2dm"])
        eng.set_params(nn, pop["beta0"])
        return eng

    def upload(eng, y):                                      # y: (1, T, N) of one replicate
        eng.set_population_cpep(pop["tp"], pop["G"], np.ascontiguousarray(y[0].T), pop["age"], pop["t2dm"])
    return dict(name="c-peptide 2-6-6-1, S = 30", make=make, upload=upload, box=(-4.0, 3.0), start=-1.0, supp=False,
                pop=np.asarray(pop["obs"], dtype=np.float64).T[None], T=len(pop["tp"]))


def supp_case(N):
    c = make_supp_case(N)

    def make():
        eng = Engine("supp", c["arch"], n_steps=30)
        eng.set_population_supp(c["tp"], c["data"])
        eng.set_params(c["nn"], np.zeros(N))
        return eng
    scale = []

    def upload(eng, y):                                      # y: (3, T, N)
        eng.set_population_supp(c["tp"], y)
        eng.set_global_subjects(N, scale[0])
    return dict(name="suppression 4-3x5-1, S = 30", make=make, upload=upload, box=(-6.0, 4.0), start=0.0, supp=True,
                pop=np.asarray(c["data"], dtype=np.float64), T=len(c["tp"]), scale=scale)


def run(case, N, B):
    eng = case["make"]()
    box, T = case["box"], case["T"]
    rows = 3 * T if case["supp"] else T
    fit = eng.refine_conditional(np.full(N, case["start"]), *box)
    center, sigma = fit["x"], np.sqrt(fit["sse"] / rows)
    sigma = np.where(np.isfinite(sigma), sigma, 0.0)
    kw = dict(ranks=[0, B // 2, B - 1], lower=box[0], upper=box[1], want_replicates=True)
    if only_launch:
        for _ in range(3 + reps):
            eng.bootstrap_conditional(sigma, B, center, **kw)
        eng.close()
        return
    scale = np.asarray(eng.get_scale()[0], dtype=np.float64) if case["supp"] else np.ones(1)
    if case["supp"]:
        case["scale"][:] = [scale]
    eng.set_params(None, center)
    traj = eng.forward(want_traj=True)["traj"]
    yhat = np.ascontiguousarray(traj if case["supp"] else traj[:1])
    noise = np.random.default_rng(5).standard_normal((B, rows, N))
    ystar = br.replicate_data(yhat, sigma, scale, noise, case["pop"])
    loop_eng = case["make"]()
    out = {}

    def loop():
        x, st, ev = np.empty((B, N)), np.empty((B, N), dtype=np.int32), np.empty((B, N), dtype=np.int32)
        for b in range(B):
            case["upload"](loop_eng, ystar[b])
            r = loop_eng.refine_conditional(center, *box)
            x[b], st[b], ev[b] = r["x"], r["status"], r["evals"]
        out["i"] = (x, st, ev)

    def launch_host():
        out["ii"] = eng.bootstrap_conditional(sigma, B, center, noise=noise, **kw)

    def launch_device():
        out["iii"] = eng.bootstrap_conditional(sigma, B, center, **kw)
    variants = [("(i)   loop of B uploads + refine", loop), ("(ii)  one launch route, host noise", launch_host),
                ("(iii) one launch route, device draws", launch_device)]
    # ---- correctness first
    loop()
    launch_host()
    x, st, ev = out["i"]
    ok = st != 4
    dx = np.abs(out["ii"]["replicates"] - x)[ok] / (1 + np.abs(x[ok]))
    same = bool(np.array_equal(out["ii"]["status"], st))
    print(f"{case['name']}, N = {N}, B = {B}: max |dx| / (1 + |x|) loop vs launch {dx.max():.2e} (bar {X_BAR:.0e}), statuses equal: "
          f"{same}, failed pairs {int(np.sum(~ok))}")
    if not (np.all(dx <= X_BAR) and same):
        raise SystemExit("the two routes disagree: no time is read")
    print(f"  evaluations per replicate fit: mean {ev[ok].mean():.2f}, max {ev[ok].max()}; status counts "
          f"{np.bincount(st.ravel(), minlength=5).tolist()} (converged, at_bound, max_evals, flat, failed)")
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
        print(f"  {k:40s} {stats(times[k])}")
    print(f"  loop / launch (host noise): {np.median(times[variants[0][0]]) / np.median(times[variants[1][0]]):.1f} x")
    eng.close()
    loop_eng.close()


for N, B in sizes:
    run(cpep_case(N), N, B)
    if not only_launch:
        run(supp_case(N), N, B)
