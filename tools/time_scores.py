"""python tools/time_scores.py  ->  profiles/scores.txt.
Wall time per cude_subject_scores call against cude_multistart_loss_grad on the same sets -- the same solves without
rows, fold, sum and cross product -- alternating, after a warm-up, on a host clock behind each call's own synchronisation:
2-6-6-1 fixed-step at 1e5 subjects and the reference's 117 subjects in adaptive mode, K = 1 (scores and cross product) and
K = 33 (the marginal gradient: weighted sets, sum and cross product only); and the K = 33 call on the fallback kernel
("force_fallback"), the only kernel that kept per-lane rows before."""
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


def run(N, K, n_steps, reps, fallback=False):
    arch = (2, 6, 2)
    c = make_cpep_case(N, arch)
    eng = Engine("cpep", arch, n_steps=n_steps, n_state=2)
    if fallback:
        eng.set_option("force_fallback", 1)
        eng.set_network([6, 6], ["tanh", "tanh", "softplus"])
    eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
    eng.set_params(c["nn"], c["beta"])
    rng = np.random.default_rng(7)
    sets = c["beta"][None, :] + 0.1 * rng.standard_normal((K, N))
    w = None if K == 1 else rng.random((K, N)) / K
    nn_sets = np.repeat(c["nn"][None, :], K, axis=0)
    want = ("scores", "cross", "sum") if K == 1 else ("sum", "cross", "wsse")

    def scores():
        return eng.subject_scores(sets, w, want=want)

    def solves():
        return eng.multistart_loss_grad(nn_sets, sets)

    scores(); solves()                            # warm-up
    ts, tm = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); scores(); t1 = time.perf_counter(); solves(); t2 = time.perf_counter()
        ts.append(t1 - t0); tm.append(t2 - t1)
    eng.close()
    print(json.dumps(dict(N=N, K=K, P=int(c["nn"].size), mode="fixed" if n_steps else "adaptive",
                          kernel="fallback" if fallback else "tuned", reps=reps,
                          subject_scores_ms_median=1e3 * float(np.median(ts)), subject_scores_ms_min=1e3 * min(ts),
                          multistart_loss_grad_ms_median=1e3 * float(np.median(tm)), multistart_loss_grad_ms_min=1e3 * min(tm))),
          flush=True)


if __name__ == "__main__":
    for N, n_steps in ((100000, 30), (117, 0)):
        run(N, 1, n_steps, 5)
        run(N, 33, n_steps, 3)
    run(100000, 33, 30, 2, fallback=True)
    run(117, 33, 0, 3, fallback=True)
