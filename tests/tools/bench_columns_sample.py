"""Times the draws of the dense-by-Kronecker blocks (gpimhip_sample_pkron) against their yardstick.

    python tests/tools/bench_columns_sample.py [--cubes 32x32x102:301,64x64x64:0.3] [--reps 3] [--yardstick-lib PATH]

The cubes of tests/tools/bench_columns.py on their own full grid; S = 1 and S = 16 draws.  Wall clock around calls that end
in a synchronise, after a warm-up call; prints the best of --reps of the library call and, from one more call with the
library's stage timers on: 6 the blocks (eigen-decomposition, factorisation, the mean's beta), 4 the prior factor, 2 the
prior draws (with the union axes and root rows), 3 the update, 5 the epilogue.
Yardstick, from --yardstick-lib (a build of the parent commit; default: this tree's library): gpimhip_predict_pkron on the
same pair of grids.
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from bench_columns import cube  # noqa: E402
from gpim_amd import _lib, _solvers, gprutils  # noqa: E402
from gpim_amd.kernels import KernelSpec  # noqa: E402

STAGES = ((6, "blocks"), (4, "prior factor"), (2, "prior draws"), (3, "update"), (5, "epilogue"))


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
    ap.add_argument("--cubes", default="32x32x102:301,64x64x64:0.3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--draws", default="1,16")
    ap.add_argument("--yardstick-lib", default=_lib.LIB_PATH)
    a = ap.parse_args()
    dev = _lib.require_gpu()
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev).contiguous()
    ylib = typed(a.yardstick_lib, ("gpimhip_create", "gpimhip_destroy", "gpimhip_predict_pkron"))
    for spec_s in a.cubes.split(","):
        dims, obs = spec_s.split(":")
        shape = tuple(int(s) for s in dims.split("x"))
        Xg, X, R = cube(shape, float(obs))
        C = gprutils.column_blocks(X, R)
        sol = _solvers.Columns(C)
        taxes = [np.arange(n, dtype=np.float64) for n in shape]
        rows, caxes, (P, iX, iT), (au, ic, it) = sol.sample_geometry(taxes)
        (Ns, J), Ms, Us = C["Y"].shape, len(rows), len(P)
        Mc, U = (int(np.prod([len(v) for v in ax])) for ax in (caxes, au))
        N, M, d = Ns * J, Ms * Mc, len(shape)
        spec = KernelSpec("RBF", d, [[2.0] * d, [12.0] * d], jitter=1e-5)
        u = spec.draw_initial_u(torch.Generator().manual_seed(3))
        u[1 + spec.n_ls] = -3.0
        m = spec.struct()
        ud, Xs_d, Y_d, ax_d = up(u.numpy()), up(C["Xs"]), up(C["Y"]), up(np.concatenate(C["axes_c"]))
        rows_d, cax_d, P_d, au_d = up(rows), up(np.concatenate(caxes)), up(P), up(np.concatenate(au))
        mean, var = torch.empty(M, dtype=torch.float64, device=dev), torch.empty(M, dtype=torch.float64, device=dev)
        model = lambda h: (h, ctypes.byref(m), _lib.ptr(Xs_d), Ns, len(C["ragged"]), len(C["complete"]),
                           i32([len(c) for c in C["axes_c"]]), i32(C["perm"]), _lib.ptr(ax_d), _lib.ptr(Y_d), _lib.ptr(ud),
                           _lib.ptr(rows_d), Ms, i32([len(c) for c in caxes]), _lib.ptr(cax_d))
        # yardstick: a prediction on the same pair of grids
        h = ctypes.c_void_p()
        assert ylib.gpimhip_create(ctypes.byref(h), dev.index, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)) == 0
        t_pred = best(lambda: _lib.check(ylib.gpimhip_predict_pkron(*model(h), _lib.ptr(mean), _lib.ptr(var))), a.reps)
        ylib.gpimhip_destroy(h)
        print("%s, %d observed pixels (N_s = %d, J = %d, N = %d) on its own grid (M = %d, U_s = %d, U = %d); "
              "gpimhip_predict_pkron (%s): %.2f ms" % (dims, Ns, Ns, J, N, M, Us, U, os.path.basename(a.yardstick_lib),
                                                      1e3 * t_pred), flush=True)
        H = _lib.Handle()
        for S in (int(s) for s in a.draws.split(",")):
            Z = torch.randn((S, Us * U + N + M), dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(S))
            out = torch.empty((S, M), dtype=torch.float64, device=dev)

            def call():
                _lib.check(H.lib.gpimhip_sample_pkron(*model(H.h), _lib.ptr(P_d), Us, i32(iX), i32(iT), i32([len(v) for v in au]),
                                                      _lib.ptr(au_d), i32(np.concatenate(ic)), i32(np.concatenate(it)),
                                                      _lib.ptr(Z), S, 0, 1e-5, _lib.ptr(mean), _lib.ptr(out)))
            whole = best(call, a.reps)
            H.lib.gpimhip_timing_enable(H.h, 1)
            call()
            st = []
            for s, label in STAGES:
                tot, cnt = ctypes.c_double(), ctypes.c_int64()
                H.lib.gpimhip_timing_read(H.h, s, ctypes.byref(tot), ctypes.byref(cnt))
                st.append("%s %.3f ms" % (label, tot.value))
            for s in (0, 1):                            # (the engine's own intervals inside stage 6: read to clear them)
                H.lib.gpimhip_timing_read(H.h, s, ctypes.byref(tot), ctypes.byref(cnt))
            H.lib.gpimhip_timing_enable(H.h, 0)
            print("  S = %d: whole call %.2f ms = %.2f x predict (%.2f x per draw); %s; workspace %.2f GiB"
                  % (S, 1e3 * whole, whole / t_pred, whole / t_pred / S, ", ".join(st),
                     H.lib.gpimhip_workspace_bytes(H.h) / 2.0 ** 30), flush=True)
            del Z, out
        H.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
