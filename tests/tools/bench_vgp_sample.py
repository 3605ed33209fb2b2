"""Times the joint draws of the multi-output GP (gpimhip_sample_vgp / gpimhip_sample_vgp_blocks).

    python tests/tools/bench_vgp_sample.py [--size 48] [--tasks 6] [--reps 3] [--train 50] [--parent-lib PATH]

The EELS twin of section 9 (size x size x tasks, Matern52, bounds [0.5, 2.5]), trained, then
  joint route   on its own grid (N = M = size^2) and on the x 2 grid (M = 4 size^2)
  blocks route  on its own grid
each with S = 1 and S = 16: best of --reps for the whole call, then one call with the library's stage timers on.
Yardstick: T calls of the single-output entry (gpimhip_sample_exact / gpimhip_sample_blocks) of --parent-lib (a build of the
parent commit; default: this tree's) at the same (N, M, S, kernel) -- what the T latent blocks cost without the multi-output
driver.  The excess over it is setup, projection, the mix kernel and the mix of the moments.  One JSON line per case; the mix
kernel is reported with its rate against the 16 T S M bytes it moves.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import gpim_amd  # noqa: E402
from bench_sample import best  # noqa: E402
from bench_sample_blocks import typed  # noqa: E402
from gpim_amd import _lib  # noqa: E402
from gpim_amd.kernels import KernelSpec  # noqa: E402
from test_gpu_vgp import eels_twin  # noqa: E402

JITTER = 1e-5


def read_stages(lib, h):
    st = {}
    for s in range(7):
        tot, cnt = ctypes.c_double(), ctypes.c_int64()
        lib.gpimhip_timing_read(h, s, ctypes.byref(tot), ctypes.byref(cnt))
        st[s] = tot.value
    return st


def parent_handle(path, dev):
    lib = typed(path, ("gpimhip_create", "gpimhip_destroy", "gpimhip_sample_exact", "gpimhip_sample_blocks"))
    h = ctypes.c_void_p()
    assert lib.gpimhip_create(ctypes.byref(h), dev.index, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)) == 0
    return lib, h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=48)
    ap.add_argument("--tasks", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--train", type=int, default=50)
    ap.add_argument("--parent-lib", default=_lib.LIB_PATH)
    a = ap.parse_args()
    dev = _lib.require_gpu()
    n, T = a.size, a.tasks
    Y = eels_twin(size=n, T=T)
    X = gpim_amd.utils.get_full_grid(Y[..., 0])
    rec = gpim_amd.vreconstructor(X, Y, kernel="Matern52", lengthscale=[0.5, 2.5], learning_rate=0.05, iterations=a.train,
                                  verbose=0)
    rec.train()
    N = n * n
    Xo, Yo = rec._observed()
    grids = {"own": Xo, "x2": torch.from_numpy(np.ascontiguousarray(
        gpim_amd.utils.get_full_grid(Y[..., 0], dense_x=0.5).reshape(2, -1).T)).to(dev).contiguous()}
    head = (rec._handle.h, ctypes.byref(rec._mstruct), ctypes.byref(rec._vstruct))
    lib = rec._handle.lib
    cshape, twoc = (ctypes.c_int32 * 2)(n, n), (ctypes.c_double * 4)(n - 1.0, n - 1.0, 0.0, 0.0)
    # the single-output model of the yardstick: the same kernel and sizes (its timings do not depend on the values)
    torch.manual_seed(3)
    spec = KernelSpec("Matern52", 2, [[0.5, 0.5], [2.5, 2.5]], jitter=JITTER)
    u1 = spec.draw_initial_u()
    u1[1 + spec.n_ls] = -1.0
    m1, u1d, y1 = spec.struct(), u1.to(dev).contiguous(), Yo[0].contiguous()
    plib, ph = parent_handle(a.parent_lib, dev)
    gen = torch.Generator(dev).manual_seed(0)
    for route, grid in (("joint", "own"), ("joint", "x2"), ("blocks", "own")):
        Xs = grids[grid]
        M = Xs.shape[0]
        W = M if route == "joint" else 3 * M
        for S in (1, 16):
            Z = torch.randn((T, S, W), dtype=torch.float64, device=dev, generator=gen)
            out = torch.empty((S, M, T), dtype=torch.float64, device=dev)
            mean, var = torch.empty((M, T), dtype=torch.float64, device=dev), torch.empty((M, T), dtype=torch.float64, device=dev)
            out1, mean1, var1 = (torch.empty((S, M), dtype=torch.float64, device=dev), torch.empty(M, dtype=torch.float64, device=dev),
                                 torch.empty(M, dtype=torch.float64, device=dev))
            if route == "joint":
                def call():
                    _lib.check(lib.gpimhip_sample_vgp(*head, _lib.ptr(Xo), _lib.ptr(Yo), N, _lib.ptr(rec._u), _lib.ptr(Xs), M,
                                                      _lib.ptr(Z), S, 0, JITTER, _lib.ptr(mean), _lib.ptr(var), _lib.ptr(out)))

                def parent():
                    for t in range(T):
                        assert plib.gpimhip_sample_exact(ph, ctypes.byref(m1), _lib.ptr(Xo), _lib.ptr(y1), N, _lib.ptr(u1d),
                                                         _lib.ptr(Xs), M, _lib.ptr(Z[t]), S, 0, JITTER, _lib.ptr(mean1),
                                                         _lib.ptr(var1), _lib.ptr(out1)) == 0
            else:
                def call():
                    _lib.check(lib.gpimhip_sample_vgp_blocks(*head, _lib.ptr(Xs), cshape, 3, twoc, _lib.ptr(Yo), _lib.ptr(rec._u),
                                                             _lib.ptr(Z), S, 0, JITTER, _lib.ptr(mean), _lib.ptr(out)))

                def parent():
                    for t in range(T):
                        assert plib.gpimhip_sample_blocks(ph, ctypes.byref(m1), _lib.ptr(Xs), cshape, 3, twoc, _lib.ptr(y1),
                                                          _lib.ptr(u1d), _lib.ptr(Z[t]), S, 0, JITTER, _lib.ptr(mean1),
                                                          _lib.ptr(out1)) == 0
            whole = best(call, a.reps)
            yard = best(parent, a.reps)
            lib.gpimhip_timing_enable(rec._handle.h, 1)
            call()
            st = read_stages(lib, rec._handle.h)
            lib.gpimhip_timing_enable(rec._handle.h, 0)
            mix_bytes = 16.0 * T * S * M
            print(json.dumps({"route": route, "grid": grid, "N": N, "M": M, "T": T, "S": S, "whole_ms": round(1e3 * whole, 3),
                              "parent_T_calls_ms": round(1e3 * yard, 3), "ratio": round(whole / yard, 4),
                              "excess_ms": round(1e3 * (whole - yard), 3),
                              "stages_ms": {"covariance": round(st[4], 3), "factorisation": round(st[0], 3),
                                            "solves": round(st[1], 3), "sweeps": round(st[5], 3),
                                            "setup_projection_or_gathers": round(st[2], 3),
                                            "moments_mix_or_rhs": round(st[3], 3), "mix_kernel": round(st[6], 4)},
                              "mix_GBps": round(mix_bytes / (st[6] * 1e-3) / 1e9, 1) if st[6] > 0 else None,
                              "workspace_GiB": round(lib.gpimhip_workspace_bytes(rec._handle.h) / 2.0 ** 30, 3),
                              "parent_lib": os.path.basename(a.parent_lib)}), flush=True)
    plib.gpimhip_destroy(ph)


if __name__ == "__main__":
    main()
