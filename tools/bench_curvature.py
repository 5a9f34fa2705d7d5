"""Wall time of cude_curvature (order-2 forward-mode solve) next to cude_sensitivity and next to the only other route to the
same number, a 4th-order central difference of four cude_sensitivity launches (cond -/+ h, -/+ 2h), on the same context and
alternating in the same process: c-peptide 2-6-6-1 fixed step, 2-4-4-1 adaptive, suppression 4-3x5-1 fixed step and
adaptive (the rows of DESIGN 7b).  Medians of perf_counter around the calls, which return after their outputs are on the
host; want_sens / want_sens2 = False, so that the three routes move the same [N] vectors.
   python tools/bench_curvature.py [N] [reps]"""
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

N = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
H = 1e-4


def report(name, eng, nn, cond):
    def curv():
        return eng.curvature(want_sens2=False)["curv"]

    def sens():
        return eng.sensitivity(want_sens=False)["info"]

    def fd4():
        s = []
        for k in (-2, -1, 1, 2):
            eng.set_params(None, cond + k * H)
            s.append(eng.sensitivity(want_sens=False)["score"])
        eng.set_params(None, cond)
        return (s[0] - 8.0 * s[1] + 8.0 * s[2] - s[3]) / (12.0 * H)

    routes = {"cude_curvature": curv, "cude_sensitivity": sens, "4 x cude_sensitivity": fd4}
    for f in routes.values():
        for _ in range(5):
            f()
    t = {k: [] for k in routes}
    for _ in range(reps):
        for k, f in routes.items():                  # alternating
            t0 = time.perf_counter()
            f()
            t[k].append(time.perf_counter() - t0)
    ms = {k: 1e3 * float(np.median(v)) for k, v in t.items()}
    a, b = curv(), fd4()
    ok = np.isfinite(a) & np.isfinite(b)
    print(f"{name} N={N}: cude_curvature {ms['cude_curvature']:.3f} ms, cude_sensitivity {ms['cude_sensitivity']:.3f} ms "
          f"(ratio {ms['cude_curvature'] / ms['cude_sensitivity']:.2f}), 4 x cude_sensitivity + 5 uploads "
          f"{ms['4 x cude_sensitivity']:.3f} ms (ratio {ms['4 x cude_sensitivity'] / ms['cude_curvature']:.2f}); "
          f"difference quotient vs curv: {np.max(np.abs(a[ok] - b[ok])) / np.max(np.abs(a[ok])):.1e} of the max-norm, "
          f"{np.count_nonzero(~ok)} non-finite", flush=True)


for arch, n_steps in (((2, 6, 2), 30), ((2, 4, 2), 0)):
    nn = bench.glorot(arch, 1234)
    eng0, pop = bench.cpep_engine(Engine, arch, 2, N, 777, 0, nn)
    eng0.close()
    eng = Engine("cpep", arch, n_steps=n_steps, n_state=2)
    eng.set_population_cpep(pop["tp"], pop["G"], pop["obs"], pop["age"], pop["t2dm"])
    eng.set_params(nn, pop["beta0"])
    report(f"c-peptide {arch} {'adaptive' if n_steps == 0 else 'fixed'}", eng, nn, np.asarray(pop["beta0"], dtype=np.float64))
    eng.close()
c = make_supp_case(N)
for n_steps in (30, 0):
    eng = Engine("supp", c["arch"], n_steps=n_steps)
    eng.set_population_supp(c["tp"], c["data"])
    eng.set_params(c["nn"], c["theta"])
    report(f"suppression {c['arch']} {'adaptive' if n_steps == 0 else 'fixed'}", eng, c["nn"], np.asarray(c["theta"], dtype=np.float64))
    eng.close()
