"""python tools/time_predictive.py  ->  profiles/predictive.txt, section 2.
cude_predictive_bands against the only route the library had before it: K x (set_params + cude_simulate) and np.sort on
the host.  Alternating, after a warm-up, at the reference's own size and at 2 000 subjects."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, d) for d in ("tests", "oracle", "conditional-ude_amd")]
import numpy as np
import torch  # noqa: F401
from conftest import make_cpep_case
from cude.engine import Engine

def run(N, K, n_times, n_steps, reps):
    arch = (2, 4, 2)
    c = make_cpep_case(N, arch)
    eng = Engine("cpep", arch, n_steps=n_steps, n_state=2)
    eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
    eng.set_params(c["nn"], c["beta"])
    times = np.linspace(c["tp"][0], c["tp"][-1], n_times)
    sets = c["beta"][None, :] + 0.4 * np.random.default_rng(4).standard_normal((K, N))
    ranks = np.unique([0, int(0.025 * (K - 1)), int(0.025 * (K - 1)) + 1, (K - 1) // 2, (K - 1) // 2 + 1, int(0.975 * (K - 1)),
                       int(0.975 * (K - 1)) + 1, K - 1]).astype(np.int32)
    def device():
        return eng.predictive_bands(sets, times, ranks, state=0)
    def host():
        v = np.empty((K, n_times, N))
        for k in range(K):
            eng.set_params(None, sets[k])
            v[k] = eng.simulate(times)[0]
        eng.set_params(None, c["beta"])
        srt = np.sort(v, axis=0)
        return {"order": srt[ranks].transpose(2, 1, 0), "mean": v.mean(axis=0).T}
    d, h = device(), host()                                   # warm-up (and the two routes agree on the order statistics)
    assert np.array_equal(d["order"], h["order"])
    td, th = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); device(); t1 = time.perf_counter(); host(); t2 = time.perf_counter()
        td.append(t1 - t0); th.append(t2 - t1)
    eng.close()
    out = dict(N=N, K=K, n_times=n_times, mode="fixed" if n_steps else "adaptive", reps=reps,
               device_ms_median=1e3 * float(np.median(td)), device_ms_min=1e3 * min(td),
               host_route_ms_median=1e3 * float(np.median(th)), host_route_ms_min=1e3 * min(th))
    print(json.dumps(out), flush=True)

if __name__ == "__main__":
    for n_steps in (30, 0):
        run(117, 200, 241, n_steps, 5)
    for n_steps in (30, 0):
        run(2000, 200, 241, n_steps, 3)
