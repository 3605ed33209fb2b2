"""Times the Kronecker posterior draws (gpimhip_sample_kron) against their yardsticks.

    python tests/tools/bench_kron_sample.py [--cases image,cube-fine,cube] [--reps 3] [--yardstick-lib PATH] [--blocks]

Cases: image 256 x 256 -> 511 x 511, cube-fine 64^3 -> 127^3, cube 64^3 on its own grid; S = 1 and S = 16 draws.  Prints the
best of --reps of the library call and, from one more call with the library's stage timers on: 0 the union axes'
eigen-decomposition, 1 the training axes' (with y~ and alpha~), 2 the prior (root rows, zeta, two chains of mode products),
3 the update (cross factors, residual, three chains of mode products), 5 the epilogue.
Yardsticks, from --yardstick-lib (a build of the parent commit; default: this tree's library):
  gpimhip_predict_kron on the same pair of grids;
  --blocks: for the cube on its own grid, gpimhip_sample_blocks (16 factorisations of order 32768, ~8 GiB per block).
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from gpim_amd import _lib, gprutils  # noqa: E402
from gpim_amd.kernels import KernelSpec  # noqa: E402

STAGES = ((0, "union eigen-decomposition"), (1, "training eigen-decomposition"), (2, "prior mode products"),
          (3, "update mode products"), (5, "epilogue"))
CASES = {
    "image": ([256, 256], lambda n: np.arange(0, n - 0.75, 0.5)),
    "cube-fine": ([64, 64, 64], lambda n: np.arange(0, n - 0.75, 0.5)),
    "cube": ([64, 64, 64], lambda n: np.arange(n, dtype=np.float64)),
}


def best(call, reps):
    call()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return min(t)


def typed(path, names):
    """`path` with the prototypes of this tree for `names` (an older build need not export every symbol of this tree)"""
    lib = ctypes.CDLL(path)
    for name in names:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib._PROTOS[name]
    return lib


def i32(v):
    return (ctypes.c_int32 * len(v))(*[int(k) for k in v])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="image,cube-fine,cube")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--yardstick-lib", default=_lib.LIB_PATH)
    ap.add_argument("--blocks", action="store_true")
    a = ap.parse_args()
    dev = _lib.require_gpu()
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev).contiguous()
    ylib = typed(a.yardstick_lib, ("gpimhip_create", "gpimhip_destroy", "gpimhip_predict_kron", "gpimhip_sample_blocks"))
    for name in a.cases.split(","):
        shape, fine = CASES[name]
        d = len(shape)
        c = [np.arange(n, dtype=np.float64) for n in shape]
        t = [fine(n) for n in shape]
        au, ic, it = gprutils.union_axes(c, t)
        N, M, PU = (int(np.prod([len(v) for v in ax])) for ax in (c, t, au))
        G = np.stack(np.meshgrid(*c, indexing="ij"), -1).reshape(-1, d)
        y = np.cos(G[:, 0] / 9.0) * np.sin(G[:, -1] / 13.0 + 0.3) + 0.05 * np.random.default_rng(0).standard_normal(N)
        spec = KernelSpec("RBF", d, [[2.0] * d, [12.0] * d], jitter=1e-5)
        u = spec.draw_initial_u(torch.Generator().manual_seed(3))
        u[1 + spec.n_ls] = -3.0
        m = spec.struct()
        ud, yd, cd, td, aud = up(u.numpy()), up(y), up(np.concatenate(c)), up(np.concatenate(t)), up(np.concatenate(au))
        mean, var = torch.empty(M, dtype=torch.float64, device=dev), torch.empty(M, dtype=torch.float64, device=dev)
        # yardstick: a prediction on the same pair of grids
        h = ctypes.c_void_p()
        assert ylib.gpimhip_create(ctypes.byref(h), dev.index, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)) == 0
        t_pred = best(lambda: _lib.check(ylib.gpimhip_predict_kron(h, ctypes.byref(m), d, i32(shape), _lib.ptr(cd), _lib.ptr(yd),
                                                                   _lib.ptr(ud), i32([len(v) for v in t]), _lib.ptr(td),
                                                                   _lib.ptr(mean), _lib.ptr(var))), a.reps)
        ylib.gpimhip_destroy(h)
        print("%s: %s -> %s (N = %d, M = %d, union grid %d points); gpimhip_predict_kron (%s): %.2f ms"
              % (name, "x".join(map(str, shape)), "x".join(str(len(v)) for v in t), N, M, PU,
                 os.path.basename(a.yardstick_lib), 1e3 * t_pred), flush=True)
        H = _lib.Handle()
        for S in (1, 16):
            Z = torch.randn((S, PU + N + M), dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(S))
            out = torch.empty((S, M), dtype=torch.float64, device=dev)

            def call():
                _lib.check(H.lib.gpimhip_sample_kron(H.h, ctypes.byref(m), d, i32(shape), _lib.ptr(cd), _lib.ptr(yd), _lib.ptr(ud),
                                                     i32([len(v) for v in t]), _lib.ptr(td), i32([len(v) for v in au]),
                                                     _lib.ptr(aud), i32(np.concatenate(ic)), i32(np.concatenate(it)), _lib.ptr(Z),
                                                     S, 0, 1e-5, _lib.ptr(mean), _lib.ptr(out)))
            whole = best(call, a.reps)
            H.lib.gpimhip_timing_enable(H.h, 1)
            call()
            st = []
            for s, label in STAGES:
                tot, cnt = ctypes.c_double(), ctypes.c_int64()
                H.lib.gpimhip_timing_read(H.h, s, ctypes.byref(tot), ctypes.byref(cnt))
                st.append("%s %.3f ms" % (label, tot.value))
            H.lib.gpimhip_timing_enable(H.h, 0)
            print("  S = %d: whole call %.2f ms = %.2f x predict (%.2f x per draw); %s; workspace %.2f GiB"
                  % (S, 1e3 * whole, whole / t_pred, whole / t_pred / S, ", ".join(st),
                     H.lib.gpimhip_workspace_bytes(H.h) / 2.0 ** 30), flush=True)
            del Z, out
        H.close()
        torch.cuda.empty_cache()
        if a.blocks and name == "cube":
            h = ctypes.c_void_p()
            assert ylib.gpimhip_create(ctypes.byref(h), dev.index, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)) == 0
            Gd = up(G)
            twoc = (ctypes.c_double * 4)(*([n - 1.0 for n in shape] + [0.0] * (4 - d)))
            for S in (1, 16):
                Z = torch.randn((S, 3 * M), dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(S))
                out = torch.empty((S, M), dtype=torch.float64, device=dev)
                t0 = time.perf_counter()
                _lib.check(ylib.gpimhip_sample_blocks(h, ctypes.byref(m), _lib.ptr(Gd), i32(shape), (1 << d) - 1, twoc, _lib.ptr(yd),
                                                      _lib.ptr(ud), _lib.ptr(Z), S, 0, 1e-5, _lib.ptr(mean), _lib.ptr(out)))
                torch.cuda.synchronize()
                print("  gpimhip_sample_blocks (%s), S = %d, one call: %.1f ms" % (os.path.basename(a.yardstick_lib), S,
                                                                                   1e3 * (time.perf_counter() - t0)), flush=True)
                del Z, out
            ylib.gpimhip_destroy(h)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
