"""vreconstructor on incomplete grids: the border solver against the dense engine.

Seconds per Adam iteration (a timed train() after a short warm-up train(), so that allocation and set-up stay outside) and
the handle's workspace bytes (Matern52, bounds [0.5, 2.5], lr 0.05; pixels removed at random with a fixed seed).  Both
solvers are forced, in the same process, alternating; "auto" is what solver=None picks.  Prints one JSON line per case.
Usage: bench_vgp_border.py [--floor] [--eels] [--large] [--profile]      (default: all three)
  --floor    the sweep behind vgpr.VGP_BORDER_MIN_OBS: square grids of side 16, 24, 32, 48, 64, T = 3, 5 % missing
  --eels     twins of the EELS stack (test_gpu_vgp.eels_twin) at 128 x 128 x 6 with 2, 5, 10 and 30 % missing
  --large    256 x 256 x 6 at 2 % missing, border only (the dense model does not fit)
  --profile  one 128 x 128 x 6, 5 % border run of 10 iterations and nothing else (for a kernel trace of its own)"""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "..")); sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import gpim_amd
from gpim_amd import gprutils
from test_gpu_vgp import eels_twin


def knock_out(X, Z, frac, seed=5):
    d, T = X.shape[0], Z.shape[-1]
    n = Z[..., 0].size
    miss = np.random.default_rng(seed).choice(n, int(round(frac * n)), replace=False)
    Xn, Zn = X.copy().reshape(d, -1), Z.copy().reshape(-1, T)
    Xn[:, miss] = np.nan
    Zn[miss] = np.nan
    return Xn.reshape(X.shape), Zn.reshape(Z.shape), len(miss)


def make(Xn, Zn, solver):
    return gpim_amd.vreconstructor(Xn, Zn, kernel="Matern52", lengthscale=[0.5, 2.5], learning_rate=0.05, iterations=2,
                                   verbose=0, solver=solver)


def timed(rec, its):
    torch.cuda.synchronize()
    t0 = time.time()
    rec.train(iterations=its)
    torch.cuda.synchronize()
    return (time.time() - t0) / its


def ws_gb(rec):
    return round(rec._handle.lib.gpimhip_workspace_bytes(rec._handle.h) / 1e9, 3)


def case(size, T, frac, its, rounds=2, dense=True):
    Z = eels_twin(size=size, T=T)
    X = gpim_amd.utils.get_full_grid(Z[..., 0])
    Xn, Zn, M = knock_out(X, Z, frac)
    fb, fd = gprutils.border_flops(size * size, M, 2)
    out = {"grid": "%dx%dx%d" % (size, size, T), "missing": frac, "M": M, "n_obs": size * size - M, "iterations": its,
           "flop_ratio": round(fb / fd, 3), "auto": make(Xn, Zn, None).solver}
    recs = {"border": make(Xn, Zn, "border")}
    if dense:
        recs["dense"] = make(Xn, Zn, "dense")
    for rec in recs.values():
        rec.train()                              # warm-up: buffers, plans
    best = {k: float("inf") for k in recs}
    for _ in range(rounds):                      # alternating; the faster of the rounds
        for k, rec in recs.items():
            best[k] = min(best[k], timed(rec, its))
    for k, rec in recs.items():
        out[k + "_s_per_iter"] = round(best[k], 6)
        out[k + "_ws_GB"] = ws_gb(rec)
    if dense:
        out["speedup"] = round(best["dense"] / best["border"], 2)
    print(json.dumps(out), flush=True)
    del recs
    torch.cuda.empty_cache()


args = set(sys.argv[1:])
if "--profile" in args:
    Z = eels_twin(size=128, T=6)
    Xn, Zn, M = knock_out(gpim_amd.utils.get_full_grid(Z[..., 0]), Z, 0.05)
    rec = make(Xn, Zn, "border")
    rec.train()
    print(json.dumps({"grid": "128x128x6", "M": M, "border_s_per_iter": round(timed(rec, 10), 6)}), flush=True)
    sys.exit(0)
run_all = not (args & {"--floor", "--eels", "--large"})
if run_all or "--floor" in args:
    for side in (16, 24, 32, 48, 64):
        case(side, 3, 0.05, 50, rounds=3)
if run_all or "--eels" in args:
    for frac in (0.02, 0.05, 0.10, 0.30):
        case(128, 6, frac, 10)
if run_all or "--large" in args:
    case(256, 6, 0.02, 4, rounds=1, dense=False)
