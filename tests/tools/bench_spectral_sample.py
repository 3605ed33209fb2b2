"""Posterior draws of the spectral-mixture GP (skreconstructor(kernel='Spectral').sample; csrc/sm.hip: sm_cross_apply_kernel,
DESIGN.md section 24) on lattice_image(size) with 25 % of the pixels observed and fully observed, Q = 4 after a short fit:
  * milliseconds of one sample() call for S = 1, 4, 16 per applicable method ('joint' only while N + M <= joint_max), next to
    predict() on the same grid in the same process -- device events around the call, one warm-up call, best of `reps`;
  * the cross-apply stage of method='pathwise' (stage timer 3: sm_cross_apply_kernel over all groups of draws plus the O(N S)
    scatter) and its kernel evaluations per second, M N Q exponentials per sweep counted from the shapes, against the same
    stage of reconstructor(kernel='Matern52').sample(method='pathwise') (cross_apply_kernel<Matern52>, M N evaluations per
    sweep) at the same M, N, S in the same run.
Usage: bench_spectral_sample.py [size=128] [fit_iterations=5] [joint_max=24000] [reps=3].  Prints one JSON line."""
import ctypes, json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "..")); sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import gpim_amd
from problems import lattice_image

size = int(sys.argv[1]) if len(sys.argv) > 1 else 128
fit_its = int(sys.argv[2]) if len(sys.argv) > 2 else 5
joint_max = int(sys.argv[3]) if len(sys.argv) > 3 else 24000
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
LS = [[1., 1.], [20., 20.]]
DRAWS = (1, 4, 16)


def timed_ms(fn):
    """Best of `reps` device-event times of fn() after one warm-up call (the first call allocates the workspaces)."""
    fn()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def stage_ms(rec, stage, fn):
    """Milliseconds the handle's stage timer `stage` collects over one call of fn() (after a warm-up call)."""
    lib, h = rec._handle.lib, rec._handle.h
    tot, cnt = ctypes.c_double(), ctypes.c_int64()
    fn()
    lib.gpimhip_timing_enable(h, 1)
    lib.gpimhip_timing_read(h, stage, ctypes.byref(tot), ctypes.byref(cnt))      # (a read clears the stage)
    fn()
    lib.gpimhip_timing_read(h, stage, ctypes.byref(tot), ctypes.byref(cnt))
    lib.gpimhip_timing_enable(h, 0)
    return tot.value


def sweeps(S):
    """Sweeps of K(G, X) for S draws: groups of up to eight (csrc/sample.hip: sample_draw_group)."""
    n, s0 = 0, 0
    while s0 < S:
        rem = S - s0
        s0 += rem if rem < 5 else min(rem, 8)
        n += 1
    return n


def measure(frac):
    R, _ = lattice_image(size, frac=frac)
    full = frac >= 1.0
    X = gpim_amd.utils.get_full_grid(R) if full else gpim_amd.utils.get_sparse_grid(R)
    Xg = gpim_amd.utils.get_full_grid(R)
    N, M, Q = int(np.sum(~np.isnan(R))), R.size, 4
    out = {"image": "%dx%d" % (size, size), "observed": frac, "N": N, "M": M, "Q": Q}
    rec = gpim_amd.skreconstructor(X, R, Xg, kernel="Spectral", n_mixtures=Q, learning_rate=0.1, iterations=fit_its, verbose=0)
    rec.train()
    out["solver"] = rec.solver
    t_pred = timed_ms(lambda: rec.predict())
    out["predict_ms"] = round(t_pred, 3)
    methods = ["pathwise"] + (["blocks"] if full else []) + (["joint"] if N + M <= joint_max else [])
    for method in methods:
        for S in DRAWS:
            t = timed_ms(lambda: rec.sample(S, seed=1, method=method))
            out["%s_S%d_ms" % (method, S)] = round(t, 3)
            out["%s_S%d_over_predict" % (method, S)] = round(t / t_pred, 3)
    mat = gpim_amd.reconstructor(X, R, Xg, kernel="Matern52", lengthscale=LS, learning_rate=0.1, iterations=fit_its, verbose=0)
    mat.train()
    for S in DRAWS:
        t_sm = stage_ms(rec, 3, lambda: rec.sample(S, seed=1, method="pathwise"))
        t_m = stage_ms(mat, 3, lambda: mat.sample(S, seed=1, method="pathwise"))
        n = sweeps(S) * M * N
        out["cross_apply_S%d" % S] = {"sm_ms": round(t_sm, 3), "sm_gevals_per_s": round(n * Q / t_sm * 1e-6, 2),
                                      "matern52_ms": round(t_m, 3), "matern52_gevals_per_s": round(n / t_m * 1e-6, 2),
                                      "sm_over_matern52_per_entry": round(t_sm / t_m, 2)}
    del rec, mat
    torch.cuda.empty_cache()
    return out


print(json.dumps({"fit_iterations": fit_its, "reps": reps, "results": [measure(f) for f in (0.25, 1.0)]}))
