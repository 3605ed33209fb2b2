"""Times the pathwise posterior draws (gpimhip_sample_pathwise) against their yardstick: the engine's
Cholesky (gpimhip_potrf) at order N plus 2^r times gpimhip_potrf at order M / 2^r.

    python tests/tools/bench_pathwise.py [--sizes 4096x12288] [--reps 3] [--kernel Matern52] [--potrf-lib PATH]

M is a complete grid (12288 = 128 x 96, 16384 = 128 x 128 with the N = 4212 pixels of the C1 scan, 65536 = 256 x 256 with the
pixels of the C2 twin; other sizes: a grid as square as M allows, N pixels at random).  Prints the whole call for S = 1 and
S = 8, the stages of the call from the library's timers (4 covariance builds, 0 factorisations, 5 the sweeps L_b z_p,
2 gathers and basis change, 1 vector solves, 3 cross_apply_kernel) and cross_apply_kernel's fp64 lane-instruction rate
against the vector rate (39.3 T lane-instructions/s), from the static instruction count of its inner loop.
--potrf-lib: another build of libgpimhip.so whose gpimhip_potrf is timed as the yardstick (a build of the parent commit);
default: this tree's.  The joint route at the same sizes: tests/tools/bench_sample.py.
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from bench_sample import best, potrf_seconds  # noqa: E402
from gpim_amd import _lib  # noqa: E402
from gpim_amd.kernels import KernelSpec  # noqa: E402

# vector instructions per covariance evaluation in cross_apply_kernel's inner loop (gfx950 ISA of this tree, SG = 1 / 8;
# RationalQuadratic goes through the device library's pow)
CROSS_APPLY_VALU = {"RBF": (33, 40), "Matern52": (45, 52), "RationalQuadratic": (404, 428)}
FP64_VECTOR_RATE = 39.3e12


def pathwise_problem(N, M, seed=0):
    """(grid shape, flat training indices, observations) of the sizes the section measures"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import problems
    if (N, M) == (4212, 16384):
        R = problems.spiral_pfm_image()
    elif (N, M) == (16384, 65536):
        R = problems.lattice_image()[0]
    else:
        a = 1 << int(np.ceil(np.log2(np.sqrt(M))))
        while M % a:
            a //= 2
        shape = (a, M // a)
        rng = np.random.default_rng(seed)
        ii, jj = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
        R = np.cos(ii / 9.0) * np.sin(jj / 13.0 + 0.3) + 0.05 * rng.standard_normal(shape)
        R.ravel()[rng.permutation(M)[N:]] = np.nan
    idx = np.flatnonzero(~np.isnan(R.ravel())).astype(np.int64)
    assert len(idx) == N and R.size == M, (len(idx), R.size)
    return R.shape, idx, R.ravel()[idx].copy()


def main_pathwise(a, dev):
    for size in a.sizes.split(","):
        N, M = (int(v) for v in size.split("x"))
        shape, idx, y = pathwise_problem(N, M)
        G = np.stack(np.unravel_index(np.arange(M), shape), axis=1).astype(np.float64)
        torch.manual_seed(3)
        spec = KernelSpec(a.kernel, 2, [[2.0, 2.0], [12.0, 12.0]], jitter=1e-5)
        u = spec.draw_initial_u()
        u[1 + spec.n_ls] = -3.0
        m = spec.struct()
        Gd, idxd, yd = (torch.from_numpy(np.ascontiguousarray(t)).to(dev).contiguous() for t in (G, idx, y))
        ud = u.to(dev).contiguous()
        cshape = (ctypes.c_int32 * 2)(*shape)
        twoc = (ctypes.c_double * 4)(shape[0] - 1.0, shape[1] - 1.0, 0.0, 0.0)
        nq = ((shape[0] + 1) // 2) * ((shape[1] + 1) // 2)
        H = _lib.Handle()
        mean = torch.empty(M, dtype=torch.float64, device=dev)
        res = {}
        for S in (1, 8):
            Z = torch.randn((S, 2 * M + N), dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(S))
            out = torch.empty((S, M), dtype=torch.float64, device=dev)

            def call():
                _lib.check(H.lib.gpimhip_sample_pathwise(H.h, ctypes.byref(m), _lib.ptr(Gd), cshape, 3, twoc,
                                                         ctypes.c_void_p(idxd.data_ptr()), _lib.ptr(yd), N, _lib.ptr(ud),
                                                         _lib.ptr(Z), S, 0, 1e-5, _lib.ptr(mean), _lib.ptr(out)))
            whole = best(call, a.reps)
            H.lib.gpimhip_timing_enable(H.h, 1)
            call()
            st = {}
            for s in (4, 0, 5, 2, 1, 3):
                tot, cnt = ctypes.c_double(), ctypes.c_int64()
                H.lib.gpimhip_timing_read(H.h, s, ctypes.byref(tot), ctypes.byref(cnt))
                st[s] = (tot.value, cnt.value)
            H.lib.gpimhip_timing_enable(H.h, 0)
            res[S] = (whole, st)
        ws_bytes = H.lib.gpimhip_workspace_bytes(H.h)
        H.close()
        torch.cuda.empty_cache()
        # the yardstick: the factorisations alone, through gpimhip_potrf of --potrf-lib
        t_y = {}
        for order in (N, nq):
            K = torch.empty((order, order), dtype=torch.float64, device=dev)
            H2 = _lib.Handle()
            XX = Gd[:order].contiguous()
            theta = torch.cat([v.reshape(-1).to(dev) for v in spec.constrained(ud)[:2]] + [torch.ones(1, dtype=torch.float64, device=dev)])
            _lib.check(H2.lib.gpimhip_kmat(H2.h, ctypes.byref(m), _lib.ptr(XX), order, None, 0, _lib.ptr(theta.contiguous()), 0.06,
                                           _lib.ptr(K), order))
            torch.cuda.synchronize()
            H2.close()
            t_y[order] = potrf_seconds(a.potrf_lib, K, a.reps)
            del K
            torch.cuda.empty_cache()
        yard = t_y[N] + 4 * t_y[nq]
        print("pathwise N = %d, M = %d (%d x %d, blocks of %d; %s): workspace %.2f GiB; gpimhip_potrf at order %d: %.2f ms, at order "
              "%d: %.2f ms -> yardstick %.2f ms (%s)" % (N, M, shape[0], shape[1], nq, a.kernel, ws_bytes / 2.0 ** 30, N,
                                                        1e3 * t_y[N], nq, 1e3 * t_y[nq], 1e3 * yard,
                                                        os.path.basename(a.potrf_lib)), flush=True)
        for S, (whole, st) in res.items():
            timed = sum(v[0] for v in st.values())
            valu = CROSS_APPLY_VALU[a.kernel][0 if S == 1 else 1]
            rate = float(M) * N * valu * st[3][1] / (st[3][0] * 1e-3)
            print("  S = %d: whole call %.2f ms = %.3f x yardstick; covariance builds %.2f ms, factorisations %.2f ms, sweeps "
                  "L_b z %.3f ms, gathers and basis change %.3f ms, vector solves %.2f ms, cross_apply %.2f ms in %d sweep(s) = "
                  "%.2f T lane-instructions/s (%.0f %% of the fp64 vector rate); outside the timed stages %.2f ms"
                  % (S, 1e3 * whole, whole / yard, st[4][0], st[0][0], st[5][0], st[2][0], st[1][0], st[3][0], st[3][1],
                     rate / 1e12, 100.0 * rate / FP64_VECTOR_RATE, 1e3 * whole - timed), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096x12288")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel", default="Matern52")
    ap.add_argument("--potrf-lib", default=_lib.LIB_PATH)
    a = ap.parse_args()
    main_pathwise(a, _lib.require_gpu())


if __name__ == "__main__":
    main()
