"""Times the border form of the reflection blocks against the dense exact GP on the observed points:
Matern52 images of 128 x 128 and 256 x 256 with 2 / 5 / 10 / 30 % of the pixels missing at random.  Prints one line per
workload: the solver skreconstructor picks, the flop models, and seconds per Adam iteration of both engines.

    python tests/tools/bench_border.py [--sizes 128,256] [--fracs 0.02,0.05,0.1,0.3] [--iters 3]
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


def image(n, frac, seed=0):
    rng = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    R = np.cos(ii / 9.0) * np.sin(jj / 13.0 + 0.3) + 0.05 * rng.standard_normal((n, n))
    R.ravel()[rng.choice(R.size, size=int(round(frac * R.size)), replace=False)] = np.nan
    return R


def per_iter(rec, iters):
    rec.train(iterations=1)            # workspace, plans, graph capture
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rec.train(iterations=iters)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--fracs", default="0.02,0.05,0.1,0.3")
    ap.add_argument("--iters", type=int, default=3)
    a = ap.parse_args()
    for n in [int(s) for s in a.sizes.split(",")]:
        for f in [float(s) for s in a.fracs.split(",")]:
            R = image(n, f)
            X = gpim_amd.utils.get_sparse_grid(R)
            S = gprutils.border_blocks(X, R)
            fb, fd = gprutils.border_flops(R.size, len(S["miss"]), len(S["dims"]))
            kw = dict(kernel="Matern52", learning_rate=0.1, iterations=1, verbose=0)
            choice = gpim_amd.skreconstructor(X, R, None, **kw).solver
            tb = per_iter(gpim_amd.reconstructor(X, R, None, structured=True, _border=S, **kw), a.iters)
            torch.cuda.empty_cache()
            td = per_iter(gpim_amd.reconstructor(X, R, None, **kw), a.iters)
            torch.cuda.empty_cache()
            print("%dx%d missing %4.1f%% (M = %d): choice %-6s  F_border/F_dense %.3f  border %.4f s  dense %.4f s  dense/border %.2f"
                  % (n, n, 100 * f, len(S["miss"]), choice, fb / fd, tb, td, td / tb), flush=True)


if __name__ == "__main__":
    main()
