"""Spectral-mixture GP on reflection blocks (skreconstructor(kernel='Spectral') on complete and nearly complete grids;
csrc/sm.hip: sm_kmat_refl_kernel / sm_grad_refl_kernel): seconds per Adam iteration at Q = 4 on
lattice_image(size) complete and with 2 % and 10 % of the pixels missing, for
  * the blocks ('reflection' / 'border', whatever the reconstructor chooses) with the stage-timer split of one loss + gradient
    evaluation: covariance build (stage 4), gradient contraction (stage 5), K^-1 product (stage 2), the rest;
  * the dense spectral-mixture path (solver='dense') of the same data;
  * Matern52 on its structured solver (skreconstructor) and on the dense engine (reconstructor), in the same process.
Usage: bench_spectral_blocks.py [iterations=10] [sizes=128,256] [dense_max=20000].  The dense models above dense_max
observations are run only for the complete image, with 2 iterations (N = 65536: three 34 GB matrices); pass dense_max=0 to
skip every dense run above 128 x 128.  Prints one JSON line."""
import ctypes, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "..")); sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import gpim_amd
from problems import lattice_image

its = int(sys.argv[1]) if len(sys.argv) > 1 else 10
sizes = [int(s) for s in sys.argv[2].split(",")] if len(sys.argv) > 2 else [128, 256]
dense_max = int(sys.argv[3]) if len(sys.argv) > 3 else 20000
LS = [[1., 1.], [20., 20.]]


def per_iter(rec, T, reps):
    """Best-of-reps seconds per Adam iteration of rec.train(iterations=T) (every call starts a fresh optimiser; the
    spectral model is put back to its initial parameters)."""
    u0 = rec._u.clone()
    best = float("inf")
    for k in range(reps + 1):           # the first call allocates the workspace (reps = 0: it is the one timed)
        rec._u.copy_(u0)
        torch.cuda.synchronize(); t0 = time.time()
        rec.train(iterations=T); torch.cuda.synchronize()
        dt = time.time() - t0
        if k > 0 or reps == 0:
            best = min(best, dt)
    return best / T


def split(rec):
    """Stage times (s) of one loss + gradient evaluation of a spectral model."""
    lib, h = rec._handle.lib, rec._handle.h
    tot, cnt = ctypes.c_double(), ctypes.c_int64()

    def stage(s_):
        lib.gpimhip_timing_read(h, s_, ctypes.byref(tot), ctypes.byref(cnt))
        return tot.value / max(cnt.value, 1) * 1e-3
    rec.nll_grad()
    lib.gpimhip_timing_enable(h, 1)
    for s_ in range(6):
        stage(s_)
    reps = 3
    torch.cuda.synchronize(); t0 = time.time()
    for _ in range(reps):
        rec.nll_grad()
    torch.cuda.synchronize(); t_eval = (time.time() - t0) / reps
    t_k, t_g, t_kinv = stage(4), stage(5), stage(2)
    lib.gpimhip_timing_enable(h, 0)
    return {"kmat": round(t_k * 1e3, 3), "grad": round(t_g * 1e3, 3), "kinv_product": round(t_kinv * 1e3, 3),
            "rest": round((t_eval - t_k - t_g - t_kinv) * 1e3, 3), "eval_timed": round(t_eval * 1e3, 3)}


def measure(size, missing):
    R, _ = lattice_image(size, frac=1.0 - missing)
    X = gpim_amd.utils.get_sparse_grid(R) if missing else gpim_amd.utils.get_full_grid(R)
    n_obs = int(np.sum(~np.isnan(R)))
    out = {"image": "%dx%d" % (size, size), "missing": missing, "N": n_obs, "Q": 4}
    sm = gpim_amd.skreconstructor(X, R, kernel="Spectral", n_mixtures=4, learning_rate=0.1, iterations=its, verbose=0)
    out["solver"] = sm.solver
    t_b = per_iter(sm, its, 2)
    out["blocks_s_per_iter"] = round(t_b, 5)
    out["blocks_split_ms"] = split(sm)
    del sm
    mat = gpim_amd.skreconstructor(X, R, kernel="Matern52", lengthscale=LS, learning_rate=0.1, iterations=its, verbose=0)
    out["matern52_solver"] = mat.solver
    t_ms = per_iter(mat, its, 2)
    out["matern52_structured_s_per_iter"] = round(t_ms, 5)
    out["blocks_over_matern52_structured"] = round(t_b / t_ms, 3)
    del mat
    torch.cuda.empty_cache()
    small = n_obs <= dense_max
    if small or (dense_max > 0 and missing == 0):
        T, reps = (its, 2) if small else (2, 0)
        smd = gpim_amd.skreconstructor(X, R, kernel="Spectral", n_mixtures=4, learning_rate=0.1, iterations=T, verbose=0,
                                       solver="dense")
        t_d = per_iter(smd, T, reps)
        out["dense_s_per_iter"] = round(t_d, 5)
        out["dense_over_blocks"] = round(t_d / t_b, 2)
        if small:
            out["dense_split_ms"] = split(smd)
        del smd
        torch.cuda.empty_cache()
    if small:
        matd = gpim_amd.reconstructor(X, R, kernel="Matern52", lengthscale=LS, learning_rate=0.1, iterations=its, verbose=0)
        t_md = per_iter(matd, its, 2)
        out["matern52_dense_s_per_iter"] = round(t_md, 5)
        out["matern52_dense_over_structured"] = round(t_md / t_ms, 2)
        del matd
        torch.cuda.empty_cache()
    return out


print(json.dumps({"iterations": its, "results": [measure(s, m) for s in sizes for m in (0.0, 0.02, 0.10)]}))
