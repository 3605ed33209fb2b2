"""Per launch class of the factorisation + inverse of ONE fit iteration, from a kernel trace joined with the launch plan as it
ran (gpimhip_step_plan_host_paired, or gpimhip_step_plan_host with GPIMHIP_NO_PAIR_STEPS=1 in the traced run):

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tests/tools/prof_fit.py 16384 3 0 Matern52
    python tools/pair_steps_trace.py DIR/.../*kernel_trace.csv 16384 [percol]

Classes: the step launches of the bulk regime (block columns whose panel leaves >= 64 columns right of it), the other step
launches, the launches after the last step.  Per class: launches, summed duration, hosted k-blocks and their rate, the time
of the solve / diagonal launches in between, and the wall time from the class's first launch to the next class's first."""
import csv
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from gpim_amd import _lib

path, N = sys.argv[1], int(sys.argv[2])
percol = len(sys.argv) > 3 and sys.argv[3] == "percol"
nb = (N + 127) // 128
lib = _lib.load()
ip = ctypes.POINTER(ctypes.c_int32)
n = ctypes.c_int64()
lead = np.zeros(nb, dtype=np.int32)
if percol:
    lib.gpimhip_step_plan_host(nb, 1, None, 0, ctypes.byref(n))
    rec = np.zeros((n.value, 6), dtype=np.int32)
    lib.gpimhip_step_plan_host(nb, 1, rec.ctypes.data_as(ip), n.value, ctypes.byref(n))
else:
    lib.gpimhip_step_plan_host_paired(nb, None, 0, ctypes.byref(n), None)
    rec = np.zeros((n.value, 6), dtype=np.int32)
    lib.gpimhip_step_plan_host_paired(nb, rec.ctypes.data_as(ip), n.value, ctypes.byref(n), lead.ctypes.data_as(ip))
rec = rec[rec[:, 5] != 5]
kblocks = np.bincount(rec[:, 0], weights=(rec[:, 4] - rec[:, 3]), minlength=nb)

rows = list(csv.DictReader(open(path)))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
name = [r["Kernel_Name"] for r in rows]
t0 = np.array([int(r["Start_Timestamp"]) for r in rows], dtype=np.int64)
t1 = np.array([int(r["End_Timestamp"]) for r in rows], dtype=np.int64)
km = [i for i, s in enumerate(name) if "kmat_kernel" in s]
lo, hi = km[-2], km[-1]                      # the last complete iteration
step = [i for i in range(lo, hi) if "chol_step_kernel" in name[i]]
fd = [i for i in range(lo, hi) if "panel_solve" in name[i] or "diag_update" in name[i]]
ids = [j for j in range(nb) if lead[j] != 2] + list(range(nb, int(rec[:, 0].max()) + 1))
assert len(ids) == len(step), (len(ids), len(step))
bulk = lambda j: j < nb and nb - (j // 4) * 4 - 4 >= 64
cls = ["bulk" if bulk(j) else ("rest" if j < nb else "post") for j in ids]
print("N = %d, %s schedule: %d step launches, iteration %.2f ms" % (N, "per-column" if percol else "paired", len(step),
                                                                  (t1[lo:hi].max() - t0[lo]) / 1e6))
for c in ("bulk", "rest", "post"):
    k = [q for q in range(len(ids)) if cls[q] == c]
    if not k:
        continue
    first, last = step[k[0]], (step[k[-1] + 1] if k[-1] + 1 < len(step) else hi)
    dur = sum(t1[step[q]] - t0[step[q]] for q in k) / 1e3
    kb = sum(kblocks[ids[q]] for q in k)
    f = [i for i in fd if first <= i < last]
    fdur = sum(t1[i] - t0[i] for i in f) / 1e3
    wall = (t0[last] - t0[first]) / 1e3 if last < len(t0) else (t1[hi - 1] - t0[first]) / 1e3
    print("%-5s %3d launches %9.1f us  %7d k-blocks %5.1f TFLOP/s | %3d solve/diag launches %7.1f us | wall %9.1f us" % (
        c, len(k), dur, kb, kb * 2 * 128 ** 3 / dur / 1e6, len(f), fdur, wall))
