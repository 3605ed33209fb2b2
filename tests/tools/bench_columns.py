"""Times the dense-by-Kronecker blocks on cubes measured at a sparse set of pixels: ms per Adam
iteration and per prediction on the full grid, for the shape of the reference's shipped cube (32 x 32 x 102 with 301
observed pixels) and for a 64^3 cube with 30 % of its columns observed -- and the dense engine on the first, which fits in
memory.  Prints one line per workload.

    python tests/tools/bench_columns.py [--cubes 32x32x102:301,64x64x64:0.3] [--iters 200] [--dense-iters 3] [--no-dense]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import gpim_amd  # noqa: E402
from gpim_amd import gprutils  # noqa: E402


def cube(shape, observed, seed=0):
    """A cube whose last axis is complete; `observed`: the number (>= 1) or the fraction (< 1) of the pixels measured."""
    rng = np.random.default_rng(seed)
    Xg = np.array(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"))
    R = np.cos(Xg[0] / 7.0) * np.sin(Xg[1] / 9.0 + 0.3) + 0.4 * np.cos(Xg[2] / 11.0) + 0.05 * rng.standard_normal(shape)
    npix = shape[0] * shape[1]
    keep = int(observed) if observed >= 1 else int(round(observed * npix))
    gone = np.ones(npix, dtype=bool)
    gone[rng.choice(npix, size=keep, replace=False)] = False
    mask = np.broadcast_to(gone.reshape(shape[0], shape[1], 1), shape)
    X = Xg.copy()
    X[:, mask] = np.nan
    R[mask] = np.nan
    return Xg, X, R


def timed(fn, reps, windows=1):
    """Seconds per call of fn: the median over `windows` timed windows of `reps` calls each, and the windows' (min, max)."""
    fn()                                # workspace, plans, graph capture
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / reps)
    return float(np.median(out)), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cubes", default="32x32x102:301,64x64x64:0.3")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--dense-iters", type=int, default=3)
    ap.add_argument("--no-dense", action="store_true")
    a = ap.parse_args()
    first = True
    for spec in a.cubes.split(","):
        dims, obs = spec.split(":")
        shape = tuple(int(s) for s in dims.split("x"))
        Xg, X, R = cube(shape, float(obs))
        C = gprutils.column_blocks(X, R)
        Ns, J = C["Y"].shape
        kw = dict(kernel="RBF", learning_rate=0.05, iterations=1, verbose=0)
        rec = gpim_amd.skreconstructor(X, R, Xg, **kw)
        # windows of a few tenths of a second at least: a.iters iterations per training call, 20 predictions
        t_it, it_lo, it_hi = (t / a.iters for t in timed(lambda: rec.train(iterations=a.iters), 1, windows=3))
        t_pr, pr_lo, pr_hi = timed(lambda: rec.predict(), 20, windows=3)
        ws = rec._handle.lib.gpimhip_workspace_bytes(rec._handle.h) / 2.0 ** 30
        line = ("%s, %d observed pixels (N_s = %d, J = %d, N = %d): solver %s  %.3f ms / Adam iteration (%.3f - %.3f)  "
                "%.2f ms / prediction of %d points (%.2f - %.2f)  workspace %.2f GiB"
                % (dims, Ns, Ns, J, Ns * J, rec.solver, 1e3 * t_it, 1e3 * it_lo, 1e3 * it_hi, 1e3 * t_pr, R.size, 1e3 * pr_lo,
                   1e3 * pr_hi, ws))
        del rec
        torch.cuda.empty_cache()
        if first and not a.no_dense:
            d = gpim_amd.reconstructor(X, R, Xg, **kw)
            t_d = timed(lambda: d.train(iterations=a.dense_iters), 1)[0] / a.dense_iters
            t_dp = timed(lambda: d.predict(), 1)[0]
            line += "  | dense engine: %.1f ms / iteration (%.0fx)  %.1f ms / prediction (%.0fx)" % (
                1e3 * t_d, t_d / t_it, 1e3 * t_dp, t_dp / t_pr)
            del d
            torch.cuda.empty_cache()
        first = False
        print(line, flush=True)


if __name__ == "__main__":
    main()
