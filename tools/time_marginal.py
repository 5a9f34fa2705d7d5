"""python tools/time_marginal.py  ->  profiles/marginal.txt.
cude_marginal_likelihood against the route a user had before it: the points formed in numpy, uploaded through
evaluate_conditional_sets(want_sse=True), the K x N SSEs downloaded and the log-sum-exp done in numpy.  Alternating, after
a warm-up: 1e5 subjects x the 33-node Gauss-Hermite rule, and the reference's 117 subjects x 2 048 device draws."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, d) for d in ("tests", "oracle", "conditional-ude_amd")]
import numpy as np
import torch  # noqa: F401
from conftest import make_cpep_case
from cude import api
from cude.engine import Engine


def run(N, K, source, n_steps, reps):
    arch = (2, 4, 2)
    c = make_cpep_case(N, arch)
    eng = Engine("cpep", arch, n_steps=n_steps, n_state=2)
    eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
    eng.set_params(c["nn"], c["beta"])
    sigma, pm, om, T = 0.4, -0.6, 0.9, len(c["tp"])
    rng = np.random.default_rng(7)
    center, scale = c["beta"] + 0.1 * rng.standard_normal(N), 0.05 + 0.3 * rng.random(N)
    z, a = api.gauss_hermite_rule(K) if source == "rule" else (None, None)

    def device():
        if source == "rule":
            return eng.marginal_likelihood(sigma, pm, om, nodes=z, log_weights=a, center=center, scale=scale)
        return eng.marginal_likelihood(sigma, pm, om, n_draws=K, center=center, scale=scale)

    def host():
        zz = np.repeat(z[:, None], N, axis=1) if source == "rule" else eng.rng_draws(0, K)[0]
        aa = a[:, None] if source == "rule" else 0.5 * np.log(2 * np.pi) - np.log(K) + 0.5 * zz * zz
        x = center[None, :] + scale[None, :] * zz
        sse = eng.evaluate_conditional_sets(x, want_sse=True)["sse"]
        t = aa - (T / 2) * np.log(sigma ** 2) - sse / (2 * sigma ** 2) - 0.5 * ((x - pm) / om) ** 2 - np.log(om) - 0.5 * np.log(2 * np.pi)
        M = t.max(axis=0)
        e = np.exp(t - M)
        S0 = e.sum(axis=0)
        m1, m2 = (e * zz).sum(axis=0) / S0, (e * zz * zz).sum(axis=0) / S0
        return {"logml": M + np.log(S0) + np.log(scale), "post_mean": center + scale * m1, "post_var": scale ** 2 * (m2 - m1 ** 2),
                "post_sse": (e * sse).sum(axis=0) / S0, "ess": S0 ** 2 / (e * e).sum(axis=0)}

    d, h = device(), host()                                   # warm-up (and the two routes agree)
    assert np.max(np.abs(d["logml"] - h["logml"])) <= 1e-10, np.max(np.abs(d["logml"] - h["logml"]))
    td, th = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); device(); t1 = time.perf_counter(); host(); t2 = time.perf_counter()
        td.append(t1 - t0); th.append(t2 - t1)
    eng.close()
    print(json.dumps(dict(N=N, K=K, source=source, mode="fixed" if n_steps else "adaptive", reps=reps,
                          device_ms_median=1e3 * float(np.median(td)), device_ms_min=1e3 * min(td),
                          host_route_ms_median=1e3 * float(np.median(th)), host_route_ms_min=1e3 * min(th))), flush=True)


if __name__ == "__main__":
    run(100000, 33, "rule", 30, 3)
    for n_steps in (30, 0):
        run(117, 2048, "draws", n_steps, 5)
