"""Times the draws on a fully observed grid (gpimhip_sample_blocks) against their yardsticks.

    python tests/tools/bench_sample_blocks.py [--sizes 128,256] [--reps 3] [--kernel Matern52] [--potrf-lib PATH]

An n x n image (n = 128: blocks of Nq = 4096 points, n = 256: Nq = 16384), S = 1 and S = 8.  Prints the whole call and its
stages from the library's timers (4 covariance builds, 0 factorisations, 5 the sweeps L_b z_p, 2 gathers and both basis
changes, 1 the multi-column solves, 3 right-hand sides, combination and epilogue).
  whole call   against 2 x 2^r x gpimhip_potrf at order Nq -- the factorisations alone
  stage 1      against stage 1 of gpimhip_sample_pathwise on a dense model with N = Nq training points (the n/2 x n/2 image,
               fully observed) and the same S: the same S + 1 solves at the same order, one vector at a time, times the 2^r
               blocks
--potrf-lib: the build of libgpimhip.so both yardsticks are taken from (a build of the parent commit); default: this tree's.
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

STAGES = (4, 0, 5, 2, 1, 3)


def read_stages(lib, h):
    st = {}
    for s in STAGES:
        tot, cnt = ctypes.c_double(), ctypes.c_int64()
        lib.gpimhip_timing_read(h, s, ctypes.byref(tot), ctypes.byref(cnt))
        st[s] = (tot.value, cnt.value)
    return st


def typed(path, names):
    """`path` with the prototypes of this tree for `names` (an older build need not export every symbol of this tree)"""
    lib = ctypes.CDLL(path)
    for name in names:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib._PROTOS[name]
    return lib


def image(n, dev):
    G = np.stack(np.unravel_index(np.arange(n * n), (n, n)), axis=1).astype(np.float64)
    y = np.cos(G[:, 0] / 9.0) * np.sin(G[:, 1] / 13.0 + 0.3) + 0.05 * np.random.default_rng(0).standard_normal(n * n)
    return (torch.from_numpy(np.ascontiguousarray(t)).to(dev).contiguous() for t in (G, y))


def pathwise_stage1(path, m, ud, n, S, dev):
    """milliseconds of stage 1 (the S + 1 vector solves) of `path`'s gpimhip_sample_pathwise on the fully observed n x n image"""
    lib = typed(path, ("gpimhip_create", "gpimhip_destroy", "gpimhip_sample_pathwise", "gpimhip_timing_enable",
                       "gpimhip_timing_read"))
    N = M = n * n
    Gd, yd = image(n, dev)
    idxd = torch.arange(N, dtype=torch.int64, device=dev)
    Z = torch.randn((S, 2 * M + N), dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(S))
    out = torch.empty((S, M), dtype=torch.float64, device=dev)
    h = ctypes.c_void_p()
    assert lib.gpimhip_create(ctypes.byref(h), dev.index, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)) == 0
    cshape, twoc = (ctypes.c_int32 * 2)(n, n), (ctypes.c_double * 4)(n - 1.0, n - 1.0, 0.0, 0.0)

    def call():
        assert lib.gpimhip_sample_pathwise(h, ctypes.byref(m), _lib.ptr(Gd), cshape, 3, twoc, ctypes.c_void_p(idxd.data_ptr()),
                                           _lib.ptr(yd), N, _lib.ptr(ud), _lib.ptr(Z), S, 0, 1e-5, None, _lib.ptr(out)) == 0
    call()
    lib.gpimhip_timing_enable(h, 1)
    call()
    ms = read_stages(lib, h)[1][0]
    lib.gpimhip_destroy(h)
    torch.cuda.empty_cache()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel", default="Matern52")
    ap.add_argument("--potrf-lib", default=_lib.LIB_PATH)
    a = ap.parse_args()
    dev = _lib.require_gpu()
    for n in (int(v) for v in a.sizes.split(",")):
        M, nq, B = n * n, (n // 2) ** 2, 4
        assert n % 2 == 0
        torch.manual_seed(3)
        spec = KernelSpec(a.kernel, 2, [[2.0, 2.0], [12.0, 12.0]], jitter=1e-5)
        u = spec.draw_initial_u()
        u[1 + spec.n_ls] = -3.0
        m = spec.struct()
        ud = u.to(dev).contiguous()
        Gd, yd = image(n, dev)
        cshape, twoc = (ctypes.c_int32 * 2)(n, n), (ctypes.c_double * 4)(n - 1.0, n - 1.0, 0.0, 0.0)
        H = _lib.Handle()
        mean = torch.empty(M, dtype=torch.float64, device=dev)
        res = {}
        for S in (1, 8):
            Z = torch.randn((S, 3 * M), dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(S))
            out = torch.empty((S, M), dtype=torch.float64, device=dev)

            def call():
                _lib.check(H.lib.gpimhip_sample_blocks(H.h, ctypes.byref(m), _lib.ptr(Gd), cshape, 3, twoc, _lib.ptr(yd),
                                                       _lib.ptr(ud), _lib.ptr(Z), S, 0, 1e-5, _lib.ptr(mean), _lib.ptr(out)))
            whole = best(call, a.reps)
            H.lib.gpimhip_timing_enable(H.h, 1)
            call()
            res[S] = (whole, read_stages(H.lib, H.h))
            H.lib.gpimhip_timing_enable(H.h, 0)
        ws_bytes = H.lib.gpimhip_workspace_bytes(H.h)
        H.close()
        torch.cuda.empty_cache()
        # yardstick of the whole call: the 2 x 2^r factorisations alone, through gpimhip_potrf of --potrf-lib
        K = torch.empty((nq, nq), dtype=torch.float64, device=dev)
        H2 = _lib.Handle()
        theta = torch.cat([v.reshape(-1).to(dev) for v in spec.constrained(ud)[:2]] + [torch.ones(1, dtype=torch.float64, device=dev)])
        _lib.check(H2.lib.gpimhip_kmat(H2.h, ctypes.byref(m), _lib.ptr(Gd[:nq].contiguous()), nq, None, 0,
                                       _lib.ptr(theta.contiguous()), 0.06, _lib.ptr(K), nq))
        torch.cuda.synchronize()
        H2.close()
        t_potrf = potrf_seconds(a.potrf_lib, K, a.reps)
        del K
        torch.cuda.empty_cache()
        yard = 2 * B * t_potrf
        print("blocks %d x %d (M = %d, %d blocks of %d; %s): workspace %.2f GiB; gpimhip_potrf at order %d: %.2f ms -> yardstick "
              "%d x = %.2f ms (%s)" % (n, n, M, B, nq, a.kernel, ws_bytes / 2.0 ** 30, nq, 1e3 * t_potrf, 2 * B, 1e3 * yard,
                                       os.path.basename(a.potrf_lib)), flush=True)
        for S, (whole, st) in res.items():
            one = B * pathwise_stage1(a.potrf_lib, m, ud, n // 2, S, dev)
            timed = sum(v[0] for v in st.values())
            print("  S = %d: whole call %.2f ms = %.3f x yardstick; covariance builds %.2f ms, factorisations %.2f ms, sweeps "
                  "L_b z %.3f ms, gathers and basis changes %.3f ms, multi-column solves %.2f ms, right-hand sides / combination / "
                  "epilogue %.3f ms; outside the timed stages %.2f ms; the solves one vector at a time (%d x stage 1 of "
                  "gpimhip_sample_pathwise at N = %d): %.2f ms -> %.2f x"
                  % (S, 1e3 * whole, whole / yard, st[4][0], st[0][0], st[5][0], st[2][0], st[1][0], st[3][0], 1e3 * whole - timed,
                     B, nq, one, one / st[1][0]), flush=True)


if __name__ == "__main__":
    main()
