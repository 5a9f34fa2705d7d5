"""Scan of the issue-priority alternation of the fixed-step gradient kernel on the bench workload (development aid):
one engine, the modes taken in turn, several rounds, so that drift of the GPU clock hits every mode alike.

usage: python tools/prio_scan.py [N=125000] [rounds=3] [steps=40] [mode ...]
  mode: off | rule | pK (progress-keyed, period 2^K evaluations) | cK (clock-keyed, period 2^K cycles)
  default modes: off rule p3 p4 p5 p6 p7 c14 c15 c16 c17 c18
  CUDE_ABL=<name>: the library variant tools/abl_so/<name>.so instead of the built one
  CUDE_SCAN_ARCH=2,4,2 CUDE_SCAN_STATES=2: another network / state count than the headline's 2,6,2 / 3
Prints per mode the median kernel time (HIP events) of every round and the median / spread over the rounds.
"""
import os
import sys

import numpy as np
import torch  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "conditional-ude_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import cude_oracle as o  # noqa: E402
from cude import _lib  # noqa: E402

if os.environ.get("CUDE_ABL"):
    _lib.LIB_PATH = os.path.join(ROOT, "tools", "abl_so", os.environ["CUDE_ABL"] + ".so")
from cude.engine import Engine  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 125000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 40
modes = sys.argv[4:] or ["off", "rule"] + [f"p{k}" for k in range(3, 8)] + [f"c{k}" for k in range(14, 19)]


def options(mode):
    if mode == "off":
        return {"prio_shift": 0, "prio_clock": 0}
    if mode == "rule":
        return {"prio_shift": -1, "prio_clock": -1}
    if mode[0] == "p":
        return {"prio_shift": int(mode[1:]), "prio_clock": 0}
    if mode[0] == "c":
        return {"prio_shift": 5, "prio_clock": int(mode[1:])}
    raise SystemExit(f"unknown mode {mode}")


arch = tuple(int(v) for v in os.environ.get("CUDE_SCAN_ARCH", "2,6,2").split(","))
n_state = int(os.environ.get("CUDE_SCAN_STATES", "3"))
tp, G, cp, age, t2, bt, rng = o.synthetic_cpep_population(N)
eng = Engine("cpep", arch, n_steps=30, n_state=n_state)
eng.set_population_cpep(tp, G, cp, age, t2)
nn = o.glorot_params(arch, 1)
eng.set_params(nn, bt)
# the bench workload (bench.py, tools/quick_bench.py): observations = the device's own solve at the true conditional
# parameters with 5 % noise, start at perturbed ones (the priority scheme's effect depends on the data: how many waves
# leave the layer-1 table, and where)
obs = eng.forward(want_traj=True)["traj"][0].T * (1 + 0.05 * rng.standard_normal((N, 5)))
obs[:, 0] = cp[:, 0]
eng.set_population_cpep(tp, G, obs, age, t2)
eng.set_params(nn, bt + 0.3 * rng.standard_normal(N))
eng.adam_init(1e-2)
for _ in range(64):                      # reach the steady GPU clock first (profiles/r02/clock_ramp.txt)
    eng.adam_step(want_loss=False)
med = {m: [] for m in modes}
for r in range(rounds):
    for m in modes:
        for name, value in options(m).items():
            try:
                eng.set_option(name, value)
            except Exception:               # a library variant from before the option: progress-keyed is all it knows
                if name != "prio_clock" or value > 0:
                    raise
        for _ in range(5):
            eng.adam_step(want_loss=False)
        eng.set_kernel_timing(True)
        for _ in range(steps):
            eng.adam_step(want_loss=False)
        med[m].append(eng.kernel_time_stats()[1])
        eng.set_kernel_timing(False)
print(f"arch={arch} states={n_state} N={N} rounds={rounds} steps={steps}: median kernel ms per round | median over rounds, max - min")
for m in modes:
    v = np.array(med[m])
    print(f"  {m:5s} " + " ".join(f"{x:.5f}" for x in v) + f" | {np.median(v):.5f} {v.max() - v.min():.5f}")
