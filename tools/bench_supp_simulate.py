"""Dense output of the suppression model (cude_simulate) at population scale: 4-3x5-1, N subjects, outputs on 0:0.1:30
(301 times), fixed-step (S = 30) and adaptive, both device layouts of the result (option "dense_layout": 0 = the
caller's [3 x T x N] written directly, 1 = lane-contiguous [T][3][N] + transpose), next to the forward-only
cude_forward launch at the 8 data times.  Prints wall times per call and the device-to-host bandwidth of a plain copy of
the same size; the kernel times come from a profiler run of this script (rocprofv3 --kernel-trace --stats).
python tools/bench_supp_simulate.py [N] [reps]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "conditional-ude_amd"))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from cude.engine import Engine  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
arch = (4, 3, 5)
tp, data, theta = bench.synthetic_suppression(N, 779)
nn = bench.glorot(arch, 1234)
grid = np.round(np.arange(0.0, 30.0 + 1e-9, 0.1), 10)
nbytes = 3 * grid.size * N * 8

# device-to-host copy of the result's size into ordinary (pageable) host memory, as cude_simulate's copy does
dev = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
host = np.empty(nbytes // 8)
ht = torch.from_numpy(host)
for _ in range(2):
    ht.copy_(dev)
torch.cuda.synchronize()
t = time.perf_counter()
for _ in range(REPS):
    ht.copy_(dev)
torch.cuda.synchronize()
copy_ms = (time.perf_counter() - t) / REPS * 1e3
print(f"N={N}: result {nbytes / 1e6:.0f} MB; plain device-to-host copy {copy_ms:.1f} ms ({nbytes / copy_ms / 1e6:.1f} GB/s)")
del dev

for n_steps in (30, 0):
    eng = Engine("supp", arch, n_steps=n_steps)
    eng.set_population_supp(tp, data)
    eng.set_params(nn, theta)
    for _ in range(3):
        eng.forward()
    t = time.perf_counter()
    for _ in range(REPS):
        eng.forward()
    fwd_ms = (time.perf_counter() - t) / REPS * 1e3
    mode = "fixed S=30" if n_steps else "adaptive"
    print(f"{mode}: cude_forward (8 data times) {fwd_ms:.3f} ms per call")
    ref = None
    for layout in (1, 0):
        eng.set_option("dense_layout", layout)
        out = eng.simulate(grid)
        if ref is None:
            ref = out
        assert np.array_equal(out, ref)
        t = time.perf_counter()
        for _ in range(REPS):
            eng.simulate(grid)
        ms = (time.perf_counter() - t) / REPS * 1e3
        print(f"{mode}: cude_simulate (301 times, layout {layout}) {ms:.1f} ms per call")
    eng.close()
