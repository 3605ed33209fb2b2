"""vreconstructor on complete grids: the reflection solver against the dense engine.

Seconds per Adam iteration (a timed train() after a short warm-up train(), so that allocation and set-up stay outside) and
the handle's workspace bytes, on twins of the reference notebook's EELS stack (test_gpu_vgp.eels_twin: Matern52, bounds
[0.5, 2.5], lr 0.05).  The dense engine gets the same points in the scattered layout.  Prints one JSON line per case.
Usage: bench_vgp_refl.py [SIZE ...]   (default: 48 96 128 256; 256 runs the reflection solver only)"""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "..")); sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import gpim_amd
from test_gpu_vgp import eels_twin, scattered

T = 6
ITERS = {48: 100, 96: 30, 128: 10, 256: 4}


def timed(X, Z, its):
    rec = gpim_amd.vreconstructor(X, Z, kernel="Matern52", lengthscale=[0.5, 2.5], learning_rate=0.05, iterations=2,
                                  verbose=0)
    rec.train()
    torch.cuda.synchronize()
    t0 = time.time()
    rec.train(iterations=its)
    torch.cuda.synchronize()
    dt = (time.time() - t0) / its
    return rec, dt


for size in [int(a) for a in sys.argv[1:]] or [48, 96, 128, 256]:
    Z = eels_twin(size=size, T=T)
    X = gpim_amd.utils.get_full_grid(Z[..., 0])
    its = ITERS.get(size, 5)
    rr, tr = timed(X, Z, its)
    out = {"grid": "%dx%dx%d" % (size, size, T), "N": size * size, "iterations": its, "solver": rr.solver,
           "refl_s_per_iter": round(tr, 5),
           "refl_ws_GB": round(rr._handle.lib.gpimhip_workspace_bytes(rr._handle.h) / 1e9, 3)}
    del rr
    torch.cuda.empty_cache()
    if size <= 128:
        Xs, Ys = scattered(X.reshape(2, -1).T, Z.reshape(-1, T))
        rd, td = timed(Xs, Ys, its)
        out.update({"dense_s_per_iter": round(td, 5),
                    "dense_ws_GB": round(rd._handle.lib.gpimhip_workspace_bytes(rd._handle.h) / 1e9, 3),
                    "speedup": round(td / tr, 2)})
        del rd
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)
