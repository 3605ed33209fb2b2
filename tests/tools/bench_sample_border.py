"""Times the draws on an image with missing pixels (gpimhip_sample_border) against their yardsticks.

    python tests/tools/bench_sample_border.py [--sizes 128,256] [--fracs 0.02,0.05] [--reps 3] [--kernel Matern52]
                                              [--parent-lib PATH] [--dense-reps 1]

An n x n image with a fraction of its pixels missing at random, S = 1 and S = 8.  Prints the whole call and its stages from
the library's timers (4 the prior's covariance builds, 0 factorisations, 5 the sweeps L_b z_p, 2 gathers and basis changes,
1 the multi-column sweeps through L_b^-1 plus what is left of the triangular inverses, 3 right-hand sides, the border's
vectors, combination and epilogue; the model's covariance build, K^-1 product and border products are not timed), and the
achieved bandwidth of the two triangular sweeps from their own timer (stage 6: one interval per group of columns, inside
stage 1's), over 2 x 2^r Nq^2 / 2 x 8 bytes per group.
  yardstick 1  one gpimhip_predict_exact_batched of the same border model on a single test chunk (128 points) plus 2^r x
               gpimhip_potrf at order Nq: the factorisations a draw cannot avoid
  yardstick 2  gpimhip_sample_pathwise of the dense model on the same data and S: what a user has without this entry
--parent-lib: the build of libgpimhip.so both yardsticks are taken from (a build of the parent commit); default: this tree's.
"""
import argparse
import ctypes
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from bench_sample import best, potrf_seconds  # noqa: E402
from bench_sample_blocks import read_stages, typed  # noqa: E402
from gpim_amd import _lib, _solvers, gprutils  # noqa: E402
from gpim_amd.kernels import KernelSpec  # noqa: E402

PARENT_SYMBOLS = ("gpimhip_create", "gpimhip_destroy", "gpimhip_last_error", "gpimhip_sample_pathwise", "gpimhip_timing_enable",
                  "gpimhip_timing_read", "gpimhip_set_reflection", "gpimhip_set_border", "gpimhip_predict_exact_batched")


def image(n, frac, dev):
    """(border blocks on the device, G (M, 2), y (M) with NaN at the missing pixels, their flat indices)"""
    M = n * n
    G = np.stack(np.unravel_index(np.arange(M), (n, n)), axis=1).astype(np.float64)
    y = np.cos(G[:, 0] / 9.0) * np.sin(G[:, 1] / 13.0 + 0.3) + 0.05 * np.random.default_rng(0).standard_normal(M)
    miss = np.sort(np.random.default_rng(1).choice(M, size=int(round(frac * M)), replace=False))
    yn = y.copy()
    yn[miss] = np.nan
    X = G.T.reshape(2, n, n).copy()
    X.reshape(2, -1)[:, miss] = np.nan
    S = gprutils.border_blocks(X, yn.reshape(n, n))
    S["n_total"] = S["n_obs"]
    D = _solvers.DeviceBlocks(S, dev)
    D.upload_border()
    return D, G, yn, miss


def raw_handle(lib, dev):
    h = ctypes.c_void_p()
    assert lib.gpimhip_create(ctypes.byref(h), dev.index, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)) == 0
    return types.SimpleNamespace(lib=lib, h=h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--fracs", default="0.02,0.05")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dense-reps", type=int, default=1)
    ap.add_argument("--kernel", default="Matern52")
    ap.add_argument("--parent-lib", "--potrf-lib", dest="parent_lib", default=_lib.LIB_PATH)
    a = ap.parse_args()
    dev = _lib.require_gpu()
    up = lambda t: torch.from_numpy(np.ascontiguousarray(t)).to(dev).contiguous()
    for n in (int(v) for v in a.sizes.split(",")):
        assert n % 2 == 0
        M, nq, B = n * n, (n // 2) ** 2, 4
        torch.manual_seed(3)
        spec = KernelSpec(a.kernel, 2, [[2.0, 2.0], [12.0, 12.0]], jitter=1e-5)
        u = spec.draw_initial_u()
        u[1 + spec.n_ls] = -3.0
        m = spec.struct()
        ud = u.to(dev).contiguous()
        ub = ud.repeat(B).contiguous()
        cshape, twoc = (ctypes.c_int32 * 2)(n, n), (ctypes.c_double * 4)(n - 1.0, n - 1.0, 0.0, 0.0)
        # 2^r x gpimhip_potrf of the parent at order Nq
        K = torch.empty((nq, nq), dtype=torch.float64, device=dev)
        H2 = _lib.Handle()
        theta = torch.cat([v.reshape(-1).to(dev) for v in spec.constrained(ud)[:2]] + [torch.ones(1, dtype=torch.float64, device=dev)])
        Gq = up(np.stack(np.unravel_index(np.arange(nq), (n // 2, n // 2)), axis=1).astype(np.float64))
        _lib.check(H2.lib.gpimhip_kmat(H2.h, ctypes.byref(m), _lib.ptr(Gq), nq, None, 0, _lib.ptr(theta.contiguous()), 0.06,
                                       _lib.ptr(K), nq))
        torch.cuda.synchronize()
        H2.close()
        t_potrf = potrf_seconds(a.parent_lib, K, a.reps)
        del K
        torch.cuda.empty_cache()
        for frac in (float(v) for v in a.fracs.split(",")):
            D, G, yn, miss = image(n, frac, dev)
            Mm = len(miss)
            Gd, missd = up(G), up(miss)
            mean = torch.empty(M, dtype=torch.float64, device=dev)
            var = torch.empty(128, dtype=torch.float64, device=dev)
            H = _lib.Handle()

            def predict(hd):
                with _lib.reflection(hd, D, 0, D.border):
                    _lib.check(hd.lib.gpimhip_predict_exact_batched(hd.h, ctypes.byref(m), _lib.ptr(D.Xq), 0, _lib.ptr(D.ys), nq, B,
                                                                    _lib.ptr(ub), _lib.ptr(Gd), 128, _lib.ptr(mean), _lib.ptr(var)))
            res = {}
            for S in (1, 8):
                Z = torch.randn((S, 3 * M), dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(S))
                out = torch.empty((S, M), dtype=torch.float64, device=dev)

                def call():
                    with _lib.reflection(H, D, 0, D.border):
                        _lib.check(H.lib.gpimhip_sample_border(H.h, ctypes.byref(m), _lib.ptr(D.Xq), 0, _lib.ptr(D.ys), nq, B,
                                                               _lib.ptr(ub), _lib.ptr(Gd), cshape, 3, twoc,
                                                               ctypes.c_void_p(missd.data_ptr()), _lib.ptr(Z), S, 0, 1e-5,
                                                               _lib.ptr(mean), _lib.ptr(out)))
                whole = best(call, a.reps)
                H.lib.gpimhip_timing_enable(H.h, 1)
                call()
                tot, cnt = ctypes.c_double(), ctypes.c_int64()
                H.lib.gpimhip_timing_read(H.h, 6, ctypes.byref(tot), ctypes.byref(cnt))
                res[S] = (whole, read_stages(H.lib, H.h), tot.value, cnt.value)
                H.lib.gpimhip_timing_enable(H.h, 0)
                del Z, out
            ws_bytes = H.lib.gpimhip_workspace_bytes(H.h)
            H.close()
            torch.cuda.empty_cache()
            # yardstick 1: the parent's prediction of the same border model on one test chunk
            plib = typed(a.parent_lib, PARENT_SYMBOLS)
            P = raw_handle(plib, dev)
            t_pred = best(lambda: predict(P), a.reps)
            plib.gpimhip_destroy(P.h)
            torch.cuda.empty_cache()
            yard1 = t_pred + B * t_potrf
            print("border %d x %d, %.0f %% missing (M = %d, %d missing -> mp = %d, %d blocks of %d; %s): workspace %.2f GiB; parent "
                  "(%s): prediction %.2f ms + %d x potrf at order %d (%.2f ms) -> yardstick 1 = %.2f ms"
                  % (n, n, 100 * frac, M, Mm, -(-Mm // 128) * 128, B, nq, a.kernel, ws_bytes / 2.0 ** 30,
                     os.path.basename(a.parent_lib), 1e3 * t_pred, B, nq, 1e3 * t_potrf, 1e3 * yard1),
                  flush=True)
            # yardstick 2: the parent's dense pathwise draw on the observed pixels
            idx = np.flatnonzero(~np.isnan(yn))
            N = len(idx)
            idxd, yd = up(idx.astype(np.int64)), up(yn[idx])
            for S, (whole, st, sweep_ms, groups) in res.items():
                if a.dense_reps > 0:
                    Z = torch.randn((S, 2 * M + N), dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(S))
                    out = torch.empty((S, M), dtype=torch.float64, device=dev)
                    P = raw_handle(plib, dev)

                    def dense():
                        assert plib.gpimhip_sample_pathwise(P.h, ctypes.byref(m), _lib.ptr(Gd), cshape, 3, twoc,
                                                            ctypes.c_void_p(idxd.data_ptr()), _lib.ptr(yd), N, _lib.ptr(ud),
                                                            _lib.ptr(Z), S, 0, 1e-5, _lib.ptr(mean), _lib.ptr(out)) == 0
                    t_dense = best(dense, a.dense_reps)
                    plib.gpimhip_destroy(P.h)
                    del Z, out
                    torch.cuda.empty_cache()
                else:
                    t_dense = float("nan")
                timed = sum(v[0] for v in st.values())
                tbs = groups * 2 * B * nq * nq / 2 * 8 / (sweep_ms * 1e-3) / 1e12 if sweep_ms > 0 else float("nan")
                print("  S = %d: whole call %.2f ms = %.3f x yardstick 1; dense pathwise (N = %d) %.1f ms -> %.2f x; covariance builds "
                      "%.2f ms, factorisations %.2f ms, sweeps L_b z %.3f ms, gathers / basis changes %.2f ms, stage 1 %.2f ms "
                      "(of which the triangular sweeps, stage 6: %.3f ms in %d group(s), %.2f TB/s), right-hand sides / border / combination %.2f ms; "
                      "outside the timed stages %.2f ms"
                      % (S, 1e3 * whole, whole / yard1, N, 1e3 * t_dense, t_dense / whole, st[4][0], st[0][0], st[5][0], st[2][0],
                         st[1][0], sweep_ms, groups, tbs, st[3][0], 1e3 * whole - timed), flush=True)


if __name__ == "__main__":
    main()
