"""Wall time of the per-subject fits: the global search against the Newton-type refinement (cude_refine_conditional).

One process, every variant warmed up, the variants alternated inside every repeat, host clock around calls that end in a
synchronisation.  Per population size and model:
  (i)   fit_conditional(41, 48) at its default fit_spec             -- the search as it stands
  (ii)  profile_conditional(41) + fused refine from the scan's argmin
  (iii) fused refine from a constant start
  (iv)  stepped refine (option refine_fused = 0; the adaptive case has no other form) from the same constant start
with mean / max evals of (ii) and (iii) and median [min, max] of the repeats in ms.

  python tools/time_refine.py [reps] [sizes ...]          (defaults: 20 repeats; 57 10000 100000)
  python tools/time_refine.py --only-fused N              one case, (iii) alone: for a rocprofv3 --kernel-trace --stats run"""
import os
import sys
import time

import numpy as np
import torch  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("conditional-ude_amd", "tests", "oracle", ""):
    sys.path.insert(0, os.path.join(ROOT, p))
import bench  # noqa: E402
from conftest import make_supp_case  # noqa: E402
from cude.engine import Engine  # noqa: E402

only_fused = "--only-fused" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = 20 if only_fused or not args else int(args[0])
sizes = [int(a) for a in (args if only_fused else args[1:])] or [57, 10000, 100000]


def cpep_case(arch, n_steps, N):
    nn = bench.glorot(arch, 1234)
    eng0, pop = bench.cpep_engine(Engine, arch, 2, N, 777, 0, nn)
    eng0.close()

    def make():
        eng = Engine("cpep", arch, n_steps=n_steps, n_state=2)
        eng.set_population_cpep(pop["tp"], pop["G"], pop["obs"], pop["age"], pop["t2dm"])
        eng.set_params(nn, pop["beta0"])
        return eng
    return make, (-4.0, 3.0), -1.0


def supp_case(N):
    c = make_supp_case(N)

    def make():
        eng = Engine("supp", c["arch"], n_steps=30)
        eng.set_population_supp(c["tp"], c["data"])
        eng.set_params(c["nn"], np.zeros(N))
        return eng
    return make, (-6.0, 4.0), 0.0


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return f"{np.median(ts):9.3f} [{ts.min():9.3f}, {ts.max():9.3f}]"


def run(name, make, box, x_const, N):
    eng, stepped = make(), make()
    stepped.set_option("refine_fused", 0)
    grid = np.linspace(box[0], box[1], 41)
    start = np.full(N, x_const)
    out = {}

    def search():
        return eng.fit_conditional(box[0], box[1], 41, 48)

    parts = {"profile launch": [], "host argmin": [], "refine": []}

    def scan_refine():
        t0 = time.perf_counter()
        prof = eng.profile_conditional(grid)
        t1 = time.perf_counter()
        x0 = grid[np.argmin(np.where(np.isfinite(prof), prof, np.inf), axis=0)]
        del prof            # as api._fit_box: the read-back array kept alive across the next call stalls it sporadically
        t2 = time.perf_counter()
        out["ii"] = eng.refine_conditional(x0, *box)
        for k, v in zip(parts, (t1 - t0, t2 - t1, time.perf_counter() - t2)):
            parts[k].append(v)

    def fused():
        out["iii"] = eng.refine_conditional(start, *box)

    def stepped_refine():
        out["iv"] = stepped.refine_conditional(start, *box)
    variants = [("(iii) fused refine, constant start", fused)] if only_fused else [
        ("(i)   search 41 + 48", search), ("(ii)  profile 41 + fused refine", scan_refine),
        ("(iii) fused refine, constant start", fused), ("(iv)  stepped refine, constant start", stepped_refine)]
    times = {k: [] for k, _ in variants}
    for _ in range(3):
        for _, f in variants:
            f()
    for v in parts.values():
        del v[:]
    for _ in range(reps):
        for k, f in variants:
            t = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t)
    print(f"{name}, N = {N}, {reps} repeats, ms: median [min, max]")
    for k, _ in variants:
        print(f"  {k:40s} {stats(times[k])}")
    if parts["refine"]:
        print("        of (ii): " + ", ".join(f"{k} {np.median(v) * 1e3:.3f}" for k, v in parts.items()))
    for k in ("ii", "iii", "iv"):
        if k in out:
            r = out[k]
            print(f"  ({k}) evals mean {r['evals'].mean():.2f} max {r['evals'].max()}, status counts "
                  f"{np.bincount(r['status'], minlength=5).tolist()} (converged, at_bound, max_evals, flat, failed)")
    if "ii" in out and not only_fused:
        xs, fs, _ = search()
        print(f"  objective, (ii) - (i): max {np.max(out['ii']['objective'] - fs):.3e}, subjects where (ii) is higher by "
              f"more than 1e-10 relative: {int(np.sum(out['ii']['objective'] > fs * (1 + 1e-10)))}")
    eng.close()
    stepped.close()


for N in sizes:
    run("c-peptide 2-6-6-1, S = 30", *cpep_case((2, 6, 2), 30, N), N)
    if only_fused:
        continue
    run("c-peptide 2-4-4-1, adaptive", *cpep_case((2, 4, 2), 0, N), N)
    run("suppression 4-3x5-1, S = 30", *supp_case(N), N)
