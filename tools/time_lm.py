"""python tools/time_lm.py  ->  profiles/lm.txt.
The second stage by Levenberg-Marquardt (cude_train_lm) against L-BFGS (cude_train_restarts with one restart and no Adam
iteration) from the same point -- the parameters after a short Adam stage -- on the 117-subject 2-6-6-1 problem (adaptive
mode) and the suppression problem (4-3x5-1, fixed-step): L-BFGS runs its budget, then LM runs until its loss is at or below
L-BFGS's final loss (or its own budget ends); iterations and wall time of both, on a host clock behind each call's own
synchronisation.  A record, not a threshold."""
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


def run(model, N, n_steps, adam_iters, lbfgs_iters, lm_iters):
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
    eng.adam_init(1e-2 if model != "supp" else 1e-3)
    eng.adam_run(adam_iters)
    nn0, cond0 = eng.get_params()
    start = eng.forward()["loss"]
    eng.train_restarts(nn0[None, :], cond0[None, :], 0, 1e-2, 2)        # warm-up of both paths
    eng.train_lm(max_iters=1)
    t0 = time.perf_counter()
    _, _, obj, trace = eng.train_restarts(nn0[None, :], cond0[None, :], 0, 1e-2, lbfgs_iters, want_trace=True)
    t_lbfgs = time.perf_counter() - t0
    n_lbfgs = int(np.count_nonzero(~np.isnan(trace[0])))
    eng.set_params(nn0, cond0)
    t0 = time.perf_counter()
    res = eng.train_lm(max_iters=lm_iters, n_trials=4, mu0=1e-2)
    t_lm = time.perf_counter() - t0
    tr = res["trace"]
    reached = np.flatnonzero(tr <= obj[0])
    n_to = int(reached[0]) if reached.size else None
    eng.close()
    print(json.dumps(dict(model=model, N=N, P=int(nn0.size), live_outputs=n_live, mode="fixed" if n_steps else "adaptive",
                          adam_iters=adam_iters, start_loss=start, lbfgs_budget=lbfgs_iters, lbfgs_iterations=n_lbfgs,
                          lbfgs_final_loss=float(obj[0]), lbfgs_wall_s=t_lbfgs, lm_budget=lm_iters, lm_iterations=res["n_iters"],
                          lm_status=res["status"], lm_final_loss=float(tr[-1]), lm_wall_s=t_lm,
                          lm_iterations_to_lbfgs_final_loss=n_to,
                          lm_wall_s_to_lbfgs_final_loss=None if n_to is None else t_lm * n_to / max(res["n_iters"], 1),
                          lm_accepted=int(np.count_nonzero(np.diff(tr) < 0.0)),
                          # five doubles of the record, the confirming loss pair, the information pass's failure count
                          device_to_host_bytes_per_lm_iteration=5 * 8 + 2 * 8 + 4)), flush=True)


if __name__ == "__main__":
    run("cpep", 117, 0, 200, 1000, 200)
    run("supp", 100, 30, 200, 1000, 200)
