"""Wall time of per-subject profile-likelihood intervals: the profile read back and reduced by numpy against
cude_profile_intervals, which keeps it on the device.

One process, every variant warmed up, the variants alternated inside every repeat, host clock around calls that end in a
synchronisation.  Per population size and model, K = 1000 scan values:
  (i)    profile_conditional(K) + numpy (threshold, first / last index inside, argmin)   -- the path as it stood
  (ii)   profile_intervals(K), no rounds                                                  -- the same scan reduced on the device
  (iii)  profile_intervals(41) + r rounds of m sections, (m + 1)^r >= (K - 1) / 40: the same end resolution from a coarse scan,
         for m = 1, 2, 4, 16
  (iv)   profile_conditional(41) + numpy argmin against profile_intervals(41, argmin only): the scan of a method = "newton" fit
with median [min, max] of the repeats in ms, and the bytes either path holds on the host and in device scratch.

  python tools/time_profile_intervals.py [reps] [sizes ...]          (defaults: 20 repeats; 57 10000 100000)"""
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

args = sys.argv[1:]
reps = int(args[0]) if args else 20
sizes = [int(a) for a in args[1:]] or [57, 10000, 100000]
K, COARSE = 1000, 41
ROUNDS = {1: 5, 2: 3, 4: 2, 16: 2}                       # m -> r with (m + 1)^r >= 999 / 40


def cpep_case(arch, n_steps, N):
    nn = bench.glorot(arch, 1234)
    eng0, pop = bench.cpep_engine(Engine, arch, 2, N, 777, 0, nn)
    eng0.close()
    eng = Engine("cpep", arch, n_steps=n_steps, n_state=2)
    eng.set_population_cpep(pop["tp"], pop["G"], pop["obs"], pop["age"], pop["t2dm"])
    eng.set_params(nn, pop["beta0"])
    return eng, (-4.0, 3.0), 2 * 0.1 ** 2 * 7.16


def supp_case(N):
    c = make_supp_case(N)
    eng = Engine("supp", c["arch"], n_steps=30)
    eng.set_population_supp(c["tp"], c["data"])
    eng.set_params(c["nn"], c["theta"])
    return eng, (-6.0, 4.0), 2 * 0.3 ** 2 * 7.16


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return f"{np.median(ts):10.3f} [{ts.min():10.3f}, {ts.max():10.3f}]"


def scratch_bytes(eng, n_points, max_sets=1):
    """Device scratch of one scan, by the library's rule: conditional sets, SSEs and partial rows of one chunk."""
    nb = (eng.N + 63) // 64
    per_point = 8.0 * (2.0 * eng.N + nb * (eng.P + 2))
    chunk = max(1, min(n_points, 32768, int(512e6 / per_point)))
    return max(chunk, max_sets) * per_point, chunk


def run(name, eng, box, delta, N):
    fine, coarse = np.linspace(box[0], box[1], K), np.linspace(box[0], box[1], COARSE)
    center = eng.get_params()[1]
    out = {}

    def host_path():
        prof = eng.profile_conditional(fine)
        eng.set_params(None, center)
        fc = eng.forward(want_sse=True)["sse"]
        inside = np.where(np.isfinite(prof), prof, np.inf) <= fc + delta
        first, last = np.argmax(inside, axis=0), K - 1 - np.argmax(inside[::-1], axis=0)
        out["i"] = (np.where(first == 0, -np.inf, fine[first]), np.where(last == K - 1, np.inf, fine[last]),
                    inside.any(axis=0))
        del prof, inside

    def device_scan():
        out["ii"] = eng.profile_intervals(fine, None, delta)

    def coarse_rounds(m):
        def f():
            out[f"iii-{m}"] = eng.profile_intervals(coarse, None, delta, rounds=ROUNDS[m], sections=m)
        return f

    def host_argmin():
        prof = eng.profile_conditional(coarse)
        out["iv-host"] = coarse[np.argmin(np.where(np.isfinite(prof), prof, np.inf), axis=0)]
        del prof

    def device_argmin():
        out["iv-dev"] = eng.profile_intervals(coarse, argmin_only=True)["argmin"]
    variants = [("(i)   profile 1000 + numpy", host_path), ("(ii)  intervals 1000, on the device", device_scan)]
    variants += [(f"(iii) intervals 41 + {ROUNDS[m]} rounds of {m}", coarse_rounds(m)) for m in ROUNDS]
    variants += [("(iv)  profile 41 + numpy argmin", host_argmin), ("(iv)  argmin only 41, on the device", device_argmin)]
    times = {k: [] for k, _ in variants}
    for _ in range(2):
        for _, f in variants:
            f()
    for _ in range(reps):
        for k, f in variants:
            t = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t)
    print(f"{name}, N = {N}, {reps} repeats, ms: median [min, max]", flush=True)
    for k, _ in variants:
        print(f"  {k:42s} {stats(times[k])}")
    ok = out["i"][2] & ((out["ii"]["status"] & 24) == 0)
    same = np.array_equal(out["i"][0][ok], out["ii"]["lower"][ok]) and np.array_equal(out["i"][1][ok], out["ii"]["upper"][ok])
    print(f"  (ii) equals (i) on the {int(ok.sum())} subjects with an interval: {same}; argmin (iv) equal: "
          f"{np.array_equal(out['iv-host'], out['iv-dev'])}")
    dev_fine, chunk = scratch_bytes(eng, K)
    dev_coarse, _ = scratch_bytes(eng, COARSE, 32)
    print(f"  bytes, host: (i) {2 * K * N * 8 + K * N:.3e} (profile, its finite copy, mask)   (ii) / (iii) {52 * N:.3e} (five doubles, three int32 per subject)")
    print(f"  bytes, device scratch: (i) {dev_fine:.3e}   (ii) {dev_fine + 16 * 8 * N:.3e}   (iii) {dev_coarse + 16 * 8 * N:.3e}"
          f"   ({chunk} scan values per launch)", flush=True)
    eng.close()


for N in sizes:
    run("c-peptide 2-6-6-1, S = 30", *cpep_case((2, 6, 2), 30, N), N)
    run("suppression 4-3x5-1, S = 30", *supp_case(N), N)
