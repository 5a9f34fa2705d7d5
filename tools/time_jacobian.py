"""python tools/time_jacobian.py  ->  profiles/jacobian.txt.
Wall time per cude_network_information call (gn, schur, coupling, dcond, status; no Jacobian to the host) against
cude_multistart_loss_grad over as many sets as the call has live outputs on the same context -- the same solves without
the fold and cross-product kernels -- alternating, after a warm-up, on a host clock behind each call's own synchronisation:
2-6-6-1 at the reference's 117 subjects in adaptive mode, 2-6-6-1 fixed-step at 1e5 subjects, and the suppression model
(4-3x5-1, fixed-step) at 1e5 subjects."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, d) for d in ("tests", "oracle", "conditional-ude_amd")]
import numpy as np
import torch  # noqa: F401
from conftest import make_cpep_case, make_supp_case
from cude.engine import Engine


def run(model, N, n_steps, reps):
    if model == "supp":
        c = make_supp_case(N, (4, 3, 5))
        eng = Engine("supp", (4, 3, 5), n_steps=n_steps)
        eng.set_population_supp(c["tp"], c["data"])
        cond, n_live = c["theta"], 2 * (len(c["tp"]) - 1)
    else:
        c = make_cpep_case(N, (2, 6, 2))
        eng = Engine("cpep", (2, 6, 2), n_steps=n_steps, n_state=2)
        eng.set_population_cpep(c["tp"], c["G"], c["obs"], c["age"], c["t2dm"])
        cond, n_live = c["beta"], len(c["tp"]) - 1
    eng.set_params(c["nn"], cond)
    nn_sets = np.repeat(c["nn"][None, :], n_live, axis=0)
    cond_sets = np.repeat(np.asarray(cond)[None, :], n_live, axis=0)

    def information():
        return eng.network_information(penalty_weight=0.1)

    def solves():
        return eng.multistart_loss_grad(nn_sets, cond_sets)

    information(); solves()                       # warm-up
    ti, tm = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); information(); t1 = time.perf_counter(); solves(); t2 = time.perf_counter()
        ti.append(t1 - t0); tm.append(t2 - t1)
    eng.close()
    print(json.dumps(dict(model=model, N=N, P=int(c["nn"].size), live_outputs=n_live, mode="fixed" if n_steps else "adaptive",
                          reps=reps, network_information_ms_median=1e3 * float(np.median(ti)),
                          network_information_ms_min=1e3 * min(ti),
                          multistart_loss_grad_ms_median=1e3 * float(np.median(tm)),
                          multistart_loss_grad_ms_min=1e3 * min(tm))), flush=True)


if __name__ == "__main__":
    run("cpep", 117, 0, 7)
    run("cpep", 100000, 30, 5)
    run("supp", 100000, 30, 5)
