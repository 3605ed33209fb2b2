"""Times one gpimhip_loo_exact call next to one gpimhip_nll_grad call of the same model: a warm handle,
the median of 10 calls, N = 4212 and 16384, double and single precision; one JSON line per case, with the bytes the
triangular passes read (for the achieved bandwidth of colsq_tri_kernel / gemv_t_tri_kernel from a kernel trace).
`--profile N`: a few calls at N only, for a run under `rocprofv3 --kernel-trace --stats`."""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from gpim_amd import _lib
from gpim_amd.kernels import KernelSpec


def problem(N):
    rng = np.random.default_rng(N)
    X = np.unique(rng.integers(0, 160, size=(N * 2, 2)), axis=0).astype(np.float64)
    rng.shuffle(X)
    X = X[:N]
    assert len(X) == N
    y = np.sin(X.sum(1) / 9.0) + 0.1 * rng.standard_normal(N)
    spec = KernelSpec("Matern52", 2, [[1., 1.], [20., 20.]], jitter=1e-5)
    u = spec.draw_initial_u(generator=torch.Generator().manual_seed(1))
    u[1 + spec.n_ls] = -3.0
    return spec, u.cuda(), torch.from_numpy(X).cuda().contiguous(), torch.from_numpy(y).cuda().contiguous()


def tri_bytes(N, rows_to, elem):
    np_ = (N + 127) // 128 * 128
    return sum((rows_to - (cb * 64 // 128) * 128) * 64 * elem for cb in range(np_ // 64) if cb * 64 < rows_to)


def run(N, precision, reps=10):
    spec, u, X, y = problem(N)
    m = spec.struct()
    H = _lib.Handle(precision=precision)
    mean, var = torch.empty(N, dtype=torch.float64, device="cuda"), torch.empty(N, dtype=torch.float64, device="cuda")
    score = torch.empty(2, dtype=torch.float64, device="cuda")
    out = torch.empty(1 + spec.n_params, dtype=torch.float64, device="cuda")
    loo = lambda: _lib.check(H.lib.gpimhip_loo_exact(H.h, ctypes.byref(m), _lib.ptr(X), _lib.ptr(y), N, _lib.ptr(u), _lib.ptr(mean),
                                                     _lib.ptr(var), _lib.ptr(score)))
    nll = lambda: _lib.check(H.lib.gpimhip_nll_grad(H.h, ctypes.byref(m), _lib.ptr(X), _lib.ptr(y), N, _lib.ptr(u),
                                                    ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(out.data_ptr() + 8)))
    res = {"N": N, "precision": precision}
    for name, fn in (("loo", loo), ("nll_grad", nll), ("loo_again", loo)):
        fn()
        fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()                                    # (the entry synchronises its stream before it returns)
            ts.append(time.perf_counter() - t0)
        res[name + "_ms"] = 1e3 * statistics.median(ts)
        res[name + "_min_ms"] = 1e3 * min(ts)
    res["score"] = score.cpu().tolist()
    elem = 4 if precision == "single" else 8
    res["colsq_bytes"] = tri_bytes(N, N, elem)
    res["gemv_bytes"] = tri_bytes(N, (N + 127) // 128 * 128, elem)
    H.close()
    return res


if __name__ == "__main__":
    if "--profile" in sys.argv:
        N = int(sys.argv[sys.argv.index("--profile") + 1])
        for precision in ("double", "single"):
            print(json.dumps(run(N, precision, reps=3)), flush=True)
        sys.exit(0)
    for N in (4212, 16384):
        for precision in ("double", "single"):
            print(json.dumps(run(N, precision)), flush=True)
