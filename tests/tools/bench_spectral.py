"""Spectral-mixture timing (skreconstructor(kernel='Spectral'), csrc/sm.hip) against the Matern52 dense iteration measured in
the same process, at two sizes: the C1 spiral mask (spiral_image(): 128 x 128, N = 4206 observed, Q = 4, d = 2) and
lattice_image(256) with 25 % observed (N = 16384).  Per size: ms per Adam iteration of both kernels (captured loop), and the
split of one SM loss + gradient evaluation from the library's stage timers: the covariance build (stage 4, lower
triangle), the gradient contraction (stage 5), the K^-1 product (stage 2) and the rest (setup, factorisation + inverse,
solves, finalize).  The kmat / grad rates use the static fp64 VALU instruction counts per entry of the d = 2 ISA
(VALU_PER_ENTRY_MIX, counted from the compiled mixture loops) against the MI355X fp64 vector peak.  Prints one JSON line."""
import ctypes, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "..")); sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import gpim_amd
from gpim_amd import _lib
from problems import spiral_image, lattice_image

its = int(sys.argv[1]) if len(sys.argv) > 1 else 20
# VALU instructions per lower entry and mixture in the d = 2 build (sm_kmat_kernel<2>: 534 per 16 entries) and contraction
# (sm_grad_kernel<2>: 137 per entry pair), counted from the compiled ISA; fp64 vector peak 78.6 TFLOP/s = 39.3e12 lane-FMA/s
VALU_PER_ENTRY_MIX = {"kmat": 534 / 16, "grad": 137 / 2}
LANE_OPS_PER_S = 39.3e12


def timed(fn, reps=3):
    best = float("inf")
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.time()
        fn(); torch.cuda.synchronize()
        best = min(best, time.time() - t0)
    return best


def measure(name, R):
    X = gpim_amd.utils.get_sparse_grid(R)
    sm = gpim_amd.skreconstructor(X, R, kernel="Spectral", learning_rate=0.1, iterations=its, verbose=0)
    N = sm.X.shape[0]
    u0 = sm._u.clone()

    def fit_sm():
        sm._u.copy_(u0); sm.scales.clear(); sm.means.clear(); sm.weights.clear(); sm.noise_all.clear(); sm.loss_all.clear()
        sm.train()
    t_sm = timed(fit_sm) / its
    t_nll = timed(lambda: sm.nll_grad())
    lib, h = sm._handle.lib, sm._handle.h
    tot, cnt = ctypes.c_double(), ctypes.c_int64()

    def stage(s_):
        lib.gpimhip_timing_read(h, s_, ctypes.byref(tot), ctypes.byref(cnt))
        return tot.value / max(cnt.value, 1)
    sm.nll_grad()
    lib.gpimhip_timing_enable(h, 1)
    for s_ in range(6):
        stage(s_)
    reps = 3
    torch.cuda.synchronize(); t0 = time.time()
    for _ in range(reps):
        sm.nll_grad()
    torch.cuda.synchronize(); t_eval = (time.time() - t0) / reps
    t_k, t_g, t_kinv = stage(4) * 1e-3, stage(5) * 1e-3, stage(2) * 1e-3
    lib.gpimhip_timing_enable(h, 0)
    mat = gpim_amd.reconstructor(X, R, kernel="Matern52", lengthscale=[[1., 1.], [20., 20.]], learning_rate=0.1,
                                 iterations=its, verbose=0)
    t_m = timed(lambda: mat.train(iterations=its)) / its
    ent = N * (N + 1) / 2
    Q = sm.num_mixtures

    def rate(name, t):
        return round(ent * Q * VALU_PER_ENTRY_MIX[name] / t / LANE_OPS_PER_S, 3)
    return {"problem": name, "N": N, "Q": Q, "d": int(sm.X.shape[1]),
            "sm_ms_per_iter": round(t_sm * 1e3, 3), "matern52_ms_per_iter": round(t_m * 1e3, 3),
            "ratio_sm_over_matern52": round(t_sm / t_m, 3), "sm_nll_grad_ms": round(t_nll * 1e3, 3),
            "split_ms": {"kmat": round(t_k * 1e3, 3), "grad": round(t_g * 1e3, 3), "kinv_product": round(t_kinv * 1e3, 3),
                         "rest": round((t_eval - t_k - t_g - t_kinv) * 1e3, 3), "eval_timed": round(t_eval * 1e3, 3)},
            "valu_per_entry_static": {k: round(v * Q, 1) for k, v in VALU_PER_ENTRY_MIX.items()},
            "fp64_vector_fraction": {"kmat": rate("kmat", t_k), "grad": rate("grad", t_g)},
            "final_loss": sm.loss_all[-1] if sm.loss_all else None}


R1, _ = spiral_image()
R2, _ = lattice_image(256, frac=0.25)
print(json.dumps({"iterations": its, "results": [measure("c1_spiral", R1), measure("lattice_256_25pct", R2)]}))
