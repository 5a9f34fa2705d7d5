"""Kernel time of cude_sensitivity (tangent-linear solve) next to the three cude_forward launches of the finite-difference
alternative (base, cond + h, cond - h) on the same context: c-peptide 2-6-6-1 fixed step, 2-4-4-1 adaptive, suppression
4-3x5-1 fixed step and adaptive.  HIP events around the ensemble launches (cude_set_kernel_timing); run it under
rocprofv3 --kernel-trace --stats to see the kernels themselves.   python tools/bench_sensitivity.py [N] [reps]"""
import os
import sys

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


def timed(eng, call, warm=10):
    for _ in range(warm):
        call()
    eng.set_kernel_timing(True)
    for _ in range(reps):
        call()
    ms, _ = eng.kernel_time_ms()
    eng.set_kernel_timing(False)
    return ms


def report(name, eng):
    fwd = timed(eng, eng.forward)
    fwd_sse = timed(eng, lambda: eng.forward(want_sse=True))
    s_all = timed(eng, eng.sensitivity)
    s_sum = timed(eng, lambda: eng.sensitivity(want_sens=False))
    ok = "meets" if s_all <= 3.0 * fwd else "MISSES"
    print(f"{name} N={N}: cude_forward {fwd:.4f} ms (with per-subject SSE {fwd_sse:.4f}), cude_sensitivity {s_all:.4f} ms "
          f"(info / score / sse only {s_sum:.4f}) = {s_all / fwd:.2f} forward launches: {ok} the three-launch condition")


for arch, n_steps in (((2, 6, 2), 30), ((2, 4, 2), 0)):
    nn = bench.glorot(arch, 1234)
    eng0, pop = bench.cpep_engine(Engine, arch, 2, N, 777, 0, nn)
    eng0.close()
    eng = Engine("cpep", arch, n_steps=n_steps, n_state=2)
    eng.set_population_cpep(pop["tp"], pop["G"], pop["obs"], pop["age"], pop["t2dm"])
    eng.set_params(nn, pop["beta0"])
    report(f"c-peptide {arch} {'adaptive' if n_steps == 0 else 'fixed'}", eng)
    eng.close()
c = make_supp_case(N)
for n_steps in (30, 0):
    eng = Engine("supp", c["arch"], n_steps=n_steps)
    eng.set_population_supp(c["tp"], c["data"])
    eng.set_params(c["nn"], c["theta"])
    report(f"suppression {c['arch']} {'adaptive' if n_steps == 0 else 'fixed'}", eng)
    eng.close()
