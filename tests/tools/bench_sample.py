"""Times the joint posterior draws of the exact GP (gpimhip_sample_exact) against its yardstick, the
engine's Cholesky (gpimhip_potrf) at the same order N + M.  Prints the whole-call time for S = 1 and S = 16, the stages
of the call (HIP events of the library's stage timers: covariance build, factorisation, forward substitution, each sweep of
the draws kernel) and the draws kernel's achieved HBM rate, one line per size.

    python tests/tools/bench_sample.py [--sizes 4096x12288] [--reps 3] [--kernel Matern52] [--potrf-lib PATH]

--potrf-lib: another build of libgpimhip.so whose gpimhip_potrf is timed as the yardstick (a build of the parent commit);
default: this tree's.
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from gpim_amd import _lib  # noqa: E402
from gpim_amd.kernels import KernelSpec  # noqa: E402


def problem(N, M, seed=0):
    """N observed and M unobserved pixels of a square image, drawn at random without replacement"""
    side = int(np.ceil(np.sqrt(N + M)))
    rng = np.random.default_rng(seed)
    pick = rng.permutation(side * side)[:N + M]
    P = np.stack(np.unravel_index(pick, (side, side)), axis=1).astype(np.float64)
    y = np.cos(P[:N, 0] / 9.0) * np.sin(P[:N, 1] / 13.0 + 0.3) + 0.05 * rng.standard_normal(N)
    return torch.from_numpy(P[:N].copy()), torch.from_numpy(y), torch.from_numpy(P[N:].copy())


def best(fn, reps):
    fn()                                    # workspace, plans
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def potrf_seconds(path, A, reps):
    """gpimhip_potrf of `path` (raw ctypes: an older build need not export every symbol of this tree) on copies of A"""
    lib = ctypes.CDLL(path)
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    lib.gpimhip_create.argtypes = [ctypes.POINTER(vp), ctypes.c_int, vp]
    lib.gpimhip_potrf.argtypes = [vp, vp, i64, i64, vp]
    lib.gpimhip_destroy.argtypes = [vp]
    h = vp()
    assert lib.gpimhip_create(ctypes.byref(h), A.device.index, vp(torch.cuda.current_stream().cuda_stream)) == 0
    n = A.shape[0]
    info = torch.zeros(1, dtype=torch.int32, device=A.device)
    W = torch.empty_like(A)

    def run():
        W.copy_(A)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert lib.gpimhip_potrf(h, vp(W.data_ptr()), n, n, vp(info.data_ptr())) == 0
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    run()
    t = min(run() for _ in range(reps))
    assert info.item() == 0
    lib.gpimhip_destroy(h)
    return t


def stages(H):
    out = {}
    for s in (4, 0, 1, 5):
        tot, cnt = ctypes.c_double(), ctypes.c_int64()
        H.lib.gpimhip_timing_read(H.h, s, ctypes.byref(tot), ctypes.byref(cnt))
        out[s] = (tot.value, cnt.value)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096x12288")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel", default="Matern52")
    ap.add_argument("--potrf-lib", default=_lib.LIB_PATH)
    a = ap.parse_args()
    dev = _lib.require_gpu()
    for size in a.sizes.split(","):
        N, M = (int(v) for v in size.split("x"))
        X, y, Xs = problem(N, M)
        torch.manual_seed(3)
        spec = KernelSpec(a.kernel, 2, [[2.0, 2.0], [12.0, 12.0]], jitter=1e-5)
        u = spec.draw_initial_u()
        u[1 + spec.n_ls] = -3.0
        m = spec.struct()
        Xd, yd, Xsd, ud = (t.to(dev).contiguous() for t in (X, y, Xs, u))
        H = _lib.Handle()
        mean = torch.empty(M, dtype=torch.float64, device=dev)
        var = torch.empty_like(mean)
        res = {}
        for S in (1, 16):
            Z = torch.randn((S, M), dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(S))
            out = torch.empty_like(Z)

            def call():
                _lib.check(H.lib.gpimhip_sample_exact(H.h, ctypes.byref(m), _lib.ptr(Xd), _lib.ptr(yd), N, _lib.ptr(ud),
                                                      _lib.ptr(Xsd), M, _lib.ptr(Z), S, 0, 1e-5, _lib.ptr(mean), _lib.ptr(var),
                                                      _lib.ptr(out)))
            whole = best(call, a.reps)
            H.lib.gpimhip_timing_enable(H.h, 1)
            call()
            st = stages(H)
            H.lib.gpimhip_timing_enable(H.h, 0)
            res[S] = (whole, st)
        ws_bytes = H.lib.gpimhip_workspace_bytes(H.h)
        H.close()
        torch.cuda.empty_cache()
        # the yardstick: the factorisation of a covariance of the same order
        K = torch.empty((N + M, N + M), dtype=torch.float64, device=dev)
        H2 = _lib.Handle()
        XX = torch.cat([Xd, Xsd]).contiguous()
        theta = torch.cat([v.reshape(-1).to(dev) for v in spec.constrained(ud)[:2]] + [torch.ones(1, dtype=torch.float64, device=dev)])
        _lib.check(H2.lib.gpimhip_kmat(H2.h, ctypes.byref(m), _lib.ptr(XX), N + M, None, 0, _lib.ptr(theta.contiguous()), 0.06,
                                       _lib.ptr(K), N + M))
        torch.cuda.synchronize()
        H2.close()
        t_potrf = potrf_seconds(a.potrf_lib, K, a.reps)
        trap = (M * N + M * (M + 1) // 2) * 8.0          # bytes of the trapezoid L[N:, :]
        tri = (M * (M + 1) // 2) * 8.0                   # ... of L22 alone (the sweeps after the first)
        print("N = %d, M = %d (order %d, %s): workspace %.2f GiB; gpimhip_potrf at order %d: %.2f ms (%s)"
              % (N, M, N + M, a.kernel, ws_bytes / 2.0 ** 30, N + M, 1e3 * t_potrf, os.path.basename(a.potrf_lib)), flush=True)
        for S, (whole, st) in res.items():
            d_ms, d_n = st[5]
            line = ("  S = %2d: whole call %.2f ms = %.3f x potrf; covariance build %.2f ms, factorisation %.2f ms, forward "
                    "substitution %.2f ms, draws %.3f ms in %d sweep(s)"
                    % (S, 1e3 * whole, whole / t_potrf, st[4][0], st[0][0], st[1][0], d_ms, d_n))
            byt = trap + (d_n - 1) * tri
            line += "; draws kernel %.2f TB/s over %.1f MB" % (byt / (d_ms * 1e-3) / 1e12, byt / 1e6)
            rest = 1e3 * whole - st[4][0] - st[0][0] - st[1][0] - d_ms
            line += "; outside the timed stages %.2f ms" % rest
            print(line, flush=True)


if __name__ == "__main__":
    main()
