"""How far two runs of the headline workload (bench.py, C2: N = 16384, Matern52, T = 100 + predict) lie apart, and the
yardstick for it: the same build against itself with the observations in another order -- like a change of the Cholesky's
schedule, only a change of the elimination order.

    python tools/traj_deviation.py run DIR [--permute SEED]     one step; writes DIR/{mean,sd,lengthscale,variance,noise}.npy
                                                                (the names of bench.py --dump-outputs)
    python tools/traj_deviation.py compare DIR_A DIR_B          max |mean|, |sd| difference; max relative difference of the
                                                                hyper-parameter histories"""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def run(out, seed):
    import torch
    import bench
    import gpim_amd
    from problems import lattice_image
    W = bench.WORKLOAD
    R, _ = lattice_image(size=W["size"], frac=W["frac"], seed=1)
    X, Xf = gpim_amd.utils.get_sparse_grid(R), gpim_amd.utils.get_full_grid(R)
    rec = gpim_amd.reconstructor(X, R, Xf, iterations=W["iterations"], verbose=0, seed=0, kernel=W["kernel"],
                                 lengthscale=W["lengthscale"], learning_rate=W["learning_rate"])
    if seed is not None:
        perm = torch.from_numpy(np.random.default_rng(seed).permutation(rec.X.shape[0])).to(rec._Xd.device)
        rec._Xd = rec._Xd[perm].contiguous()
        rec._yd = rec._yd[perm].contiguous()
    rec.train()
    rec.predict()
    mean, sd = (t.detach().cpu().numpy() for t in rec._last_pred)
    os.makedirs(out, exist_ok=True)
    np.save(os.path.join(out, "mean.npy"), mean)
    np.save(os.path.join(out, "sd.npy"), sd)
    for k in ("lengthscale", "variance", "noise"):
        np.save(os.path.join(out, k + ".npy"), np.asarray(rec.hyperparams[k][-W["iterations"]:], dtype=np.float64))


def compare(a, b):
    d = {}
    for k in ("mean", "sd"):
        d[k] = float(np.nanmax(np.abs(np.load(os.path.join(a, k + ".npy")).ravel() - np.load(os.path.join(b, k + ".npy")).ravel())))
    hyp = 0.0
    for k in ("lengthscale", "variance", "noise"):
        x, y = np.load(os.path.join(a, k + ".npy")), np.load(os.path.join(b, k + ".npy"))
        hyp = max(hyp, float(np.max(np.abs(x - y) / np.abs(y))))
    print("%s vs %s: max |mean diff| %.3e, max |sd diff| %.3e, max rel. diff of the hyper-parameter histories %.3e" % (
        a, b, d["mean"], d["sd"], hyp))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], int(sys.argv[4]) if len(sys.argv) > 4 and sys.argv[3] == "--permute" else None)
    else:
        compare(sys.argv[2], sys.argv[3])
