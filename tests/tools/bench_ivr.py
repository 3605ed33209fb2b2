"""Times one gpimhip_ivr_exact call next to one gpimhip_predict_exact call of the same model and grid:
a warm handle, a host clock around a call that ends in a synchronise, the median of 10 calls, (N, M) = (1024, 4096) and
(4212, 16384); one JSON line per case, with the flop of the TN product and the bytes the symmetric pass reads (for the
achieved rates from a kernel trace).
`--profile N M`: a few calls at (N, M) only, with one gpimhip_loo_exact call so that colsq_tri_kernel<double> shows in the
same trace, for a run under `rocprofv3 --kernel-trace --stats`."""
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


def problem(N, M):
    rng = np.random.default_rng(N)
    X = np.unique(rng.integers(0, 160, size=(N * 2, 2)), axis=0).astype(np.float64)
    rng.shuffle(X)
    X = X[:N]
    assert len(X) == N
    y = np.sin(X.sum(1) / 9.0) + 0.1 * rng.standard_normal(N)
    n = int(round(M ** 0.5))
    assert n * n == M
    ax = np.linspace(0.0, 159.0, n)
    G = np.stack([g.reshape(-1) for g in np.meshgrid(ax, ax, indexing="ij")], axis=1)
    spec = KernelSpec("Matern52", 2, [[1., 1.], [20., 20.]], jitter=1e-5)
    u = spec.draw_initial_u(generator=torch.Generator().manual_seed(1))
    u[1 + spec.n_ls] = -3.0
    return spec, u.cuda(), torch.from_numpy(X).cuda().contiguous(), torch.from_numpy(y).cuda().contiguous(), \
        torch.from_numpy(np.ascontiguousarray(G)).cuda()


def run(N, M, reps=10, with_loo=False):
    spec, u, X, y, G = problem(N, M)
    m = spec.struct()
    H = _lib.Handle()
    mean, sd, acq = (torch.empty(M, dtype=torch.float64, device="cuda") for _ in range(3))
    head = (H.h, ctypes.byref(m), _lib.ptr(X), _lib.ptr(y), N, _lib.ptr(u))
    ivr = lambda: _lib.check(H.lib.gpimhip_ivr_exact(*head, _lib.ptr(G), M, None, None, _lib.ptr(mean), _lib.ptr(sd), _lib.ptr(acq)))
    pred = lambda: _lib.check(H.lib.gpimhip_predict_exact(*head, _lib.ptr(G), M, _lib.ptr(mean), _lib.ptr(sd)))
    res = {"N": N, "M": M}
    for name, fn in (("ivr", ivr), ("predict", pred), ("ivr_again", ivr)):
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
    if with_loo:
        lm, lv = torch.empty(N, dtype=torch.float64, device="cuda"), torch.empty(N, dtype=torch.float64, device="cuda")
        score = torch.empty(2, dtype=torch.float64, device="cuda")
        for _ in range(3):
            _lib.check(H.lib.gpimhip_loo_exact(*head, _lib.ptr(lm), _lib.ptr(lv), _lib.ptr(score)))
    res["acq_max"] = float(acq.max().item())
    nt, nb = (M + 127) // 128, (N + 127) // 128
    res["tn_flop"] = 2.0 * (nt * (nt + 1) // 2) * 128 * 128 * nb * 128
    # stored tiles of C, the upper halves of the diagonal tiles' 32-column groups skipped (ivr.hip: colsq_sym_kernel)
    res["colsq_sym_bytes"] = 8 * (nt * (nt - 1) // 2 * 128 * 128 + nt * sum(32 for rr in range(8) for cc in range(4) if 16 * rr + 15 >= 32 * cc) * 16)
    np_ = nb * 128
    res["colsq_tri_bytes"] = sum((N - (cb * 64 // 128) * 128) * 64 * 8 for cb in range(np_ // 64) if cb * 64 < N)
    res["workspace_bytes"] = int(H.lib.gpimhip_workspace_bytes(H.h))
    H.close()
    return res


if __name__ == "__main__":
    if "--profile" in sys.argv:
        i = sys.argv.index("--profile")
        print(json.dumps(run(int(sys.argv[i + 1]), int(sys.argv[i + 2]), reps=3, with_loo=True)), flush=True)
        sys.exit(0)
    for N, M in ((1024, 4096), (4212, 16384)):
        print(json.dumps(run(N, M)), flush=True)
