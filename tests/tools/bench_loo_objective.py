"""Times one gpimhip_loo_grad call next to one gpimhip_nll_grad call of the same model: a warm handle,
the host clock around a call that ends in a stream synchronise, the median of 10 calls, one process; N = 4212 and 16384,
Matern52, d = 2, double precision; one JSON line per N with the two times, their ratio and the flop of the new product
(lower tiles of C C^T at full k-range, padded order) for the launch's TFLOP/s from a kernel trace.
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


def run(N, reps=10):
    spec, u, X, y = problem(N)
    m = spec.struct()
    H = _lib.Handle()
    outs = {k: torch.empty(1 + spec.n_params, dtype=torch.float64, device="cuda") for k in ("loo_grad", "nll_grad")}

    def call(name):
        out = outs[name]
        fn = H.lib.gpimhip_loo_grad if name == "loo_grad" else H.lib.gpimhip_nll_grad
        _lib.check(fn(H.h, ctypes.byref(m), _lib.ptr(X), _lib.ptr(y), N, _lib.ptr(u), ctypes.c_void_p(out.data_ptr()),
                      ctypes.c_void_p(out.data_ptr() + 8)))

    res = {"N": N}
    for name in ("nll_grad", "loo_grad", "nll_grad_again"):
        entry = name.replace("_again", "")
        call(entry)
        call(entry)
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call(entry)                             # (the entry synchronises its stream before it returns)
            ts.append(time.perf_counter() - t0)
        res[name + "_ms"] = 1e3 * statistics.median(ts)
        res[name + "_min_ms"] = 1e3 * min(ts)
    res["ratio"] = res["loo_grad_ms"] / res["nll_grad_ms"]
    nb = (N + 127) // 128
    res["cct_flop"] = nb * (nb + 1) // 2 * 2 * 128 * 128 * (nb * 128)
    res["loss"] = {k: v[0].item() for k, v in outs.items()}
    H.close()
    return res


if __name__ == "__main__":
    if "--profile" in sys.argv:
        print(json.dumps(run(int(sys.argv[sys.argv.index("--profile") + 1]), reps=3)), flush=True)
        sys.exit(0)
    for N in (4212, 16384):
        print(json.dumps(run(N)), flush=True)
