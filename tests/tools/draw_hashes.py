"""Prints the SHA-256 of what the public sample() / predict() calls return on a fixed set of small cases, one line per case.

    python tests/tools/draw_hashes.py

For refactors of the draw and prediction drivers that must not change a bit: run it on the commit before and on the commit
after, on the same machine, and diff the two printouts by hand.  It compares nothing and stores nothing.  The models are
not trained before their draws and predictions (the hyper-parameters are the seeded initial ones; a model's training case
comes last); every draw takes S = 9 samples, two draw groups (8 + 1), unless its line says otherwise.
The cases, each for a branch of csrc/draws.hip, the prediction loops of csrc/api.hip, the spectral-mixture, multi-output and
dense-by-Kronecker drivers (csrc/smgp.hip, vgpgp.hip, pkrongp.hip), the drivers and workspaces of csrc/kron.hip or the panel
drivers of csrc/distgp.hip:
  joint      N = 300, M = 340 (the training rows end in block row 3 of 5) with an explicit z; N = 40, M = 20 (one block)
  pathwise   48 x 48 grid, both axes reflected (576-point blocks: two panels), 600 observed pixels; with noise and noiseless
  blocks     the same grid, fully observed;  border: the same grid with 5 missing pixels
  vgp        T = 2 outputs on a 16 x 16 grid: joint and blocks
  spectral   Q = 2 mixtures on a 16 x 16 grid: joint, pathwise and blocks
  columns    a (48, 6, 5) cube, 37 of the 48 rows along the first axis observed, drawn and predicted at 11 new rows times the
             training axes (the union axes are the training axes), and with new coordinates on one complete axis; both draws
             again with S = 10 and GPIMHIP_PKRON_DRAW_GROUP=4 (groups of 4, 4 and 2: the same bits as one group of 10);
             nll_grad and ten Adam iterations
  kron       a fully observed 12 x 10 grid: drawn and predicted on itself, drawn on the half-step grid (the union axes are
             not the training axes: the second decomposition), nll_grad and ten Adam iterations
  dist       N = 700 on one device: gpimhip_dist_begin to the factor, its log det and a forward / backward solve
  sm, vgp    Q = 2 mixtures / T = 2 outputs on a 16 x 16 grid in three regimes each (dense: 200 observed pixels for sm, the
             dense solver for vgp; blocks: the complete grid; border: 3 missing pixels): predict, nll_grad, ten Adam
             iterations; gpimhip_sm_kmat on a dense handle and in reflection mode; two predictions at M = 961 and the two
             stationary dense ones through the slab path (GPIMHIP_NO_FUSED_PREDICT)
  stationary the training launches of csrc/grad.hip: the dense model at N = 300 (RBF, Matern52, RationalQuadratic in double,
             RBF in single) and the reflection blocks of a 16 x 16 grid (Matern52, structured=True), nll_grad and ten Adam
             iterations each; fit_predict_batch of three data sets of N = 300 (8 iterations); rec.loo() on the dense model;
             expected improvement and gpimhip_topk at M = 340 (the single-workgroup ranking)
  acquire    the N = 300 / M = 340 data again: gpimhip_acquire_exact for cb / ei / poi, with and without a 1 / NaN mask, fused
             and through the slab path; gpimhip_acq for the three kinds; rec.ivr(), rec.ivr_batch(4) and rec.acq_batch(4, kind)
             (points, values and the four maps); three boptimizer steps with batch_update=True for the thinned batch,
             ivr_batch='greedy' and acq_batch='believer' (indices and values); gpimhip_topk at M = 5000, k = 10 (radix) and
             gpimhip_nanmax at n = 5000 (two-stage) on a seeded vector
"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import gpim_amd  # noqa: E402

S = 9
LS2 = [[1., 1.], [8., 8.]]


def sha(*arrays):
    return " ".join(hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest() for a in arrays)


def image(shape, n_obs=None, seed=0):
    """(y with NaN at the unobserved pixels, the full image)"""
    rng = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    full = np.sin(ii / 3.0) * np.cos(jj / 4.0) + 0.05 * rng.standard_normal(shape)
    R = full.copy()
    if n_obs is not None:
        R.ravel()[rng.permutation(full.size)[n_obs:]] = np.nan
    return R, full


def grid(*axes):
    return np.array(np.meshgrid(*axes, indexing="ij"))


def sparse_and_full(R):
    return gpim_amd.utils.get_sparse_grid(R), gpim_amd.utils.get_full_grid(R)


def columns_cube():
    """(X with NaN, y with NaN) of a (48, 6, 5) cube with 37 of the 48 rows along axis 0 observed"""
    rng = np.random.default_rng(1)
    Xg = grid(np.arange(48.0), np.arange(6.0), np.arange(5.0))
    y = np.cos(Xg[0] / 7.0) * np.sin(Xg[1] / 2.0 + 0.3) + 0.4 * np.cos(Xg[2] / 2.5) + 0.05 * rng.standard_normal(Xg.shape[1:])
    gone = rng.permutation(48)[37:]
    X = Xg.copy()
    X[:, gone] = np.nan
    y[gone] = np.nan
    return X, y


def cases():
    """(name, thunk returning the arrays to hash) in a fixed order"""
    kw = dict(lengthscale=LS2, verbose=0)
    # ---- joint
    R, _ = image((20, 17), 300)
    Xs, Xf = sparse_and_full(R)
    r = gpim_amd.reconstructor(Xs, R, Xf, kernel="Matern52", **kw)
    z = np.random.default_rng(5).standard_normal((S, 340))
    yield "joint N=300 M=340", lambda: (r.sample(S, z=z),)
    yield "joint N=300 M=340 noiseless", lambda: (r.sample(S, z=z, noiseless=True),)
    yield "predict N=300 M=340", lambda: r.predict(verbose=0)
    _, full = image((8, 5))
    r1 = gpim_amd.reconstructor(gpim_amd.utils.get_full_grid(full), full, grid(np.arange(5) + 0.5, np.arange(4) + 0.25),
                                kernel="RBF", **kw)
    yield "joint N=40 M=20", lambda: (r1.sample(S, seed=3),)
    # ---- pathwise, blocks, border on a 48 x 48 grid
    R, full = image((48, 48), 600)
    Xs, Xf = sparse_and_full(R)
    rp = gpim_amd.reconstructor(Xs, R, Xf, kernel="Matern52", **kw)
    yield "pathwise 48x48 N=600", lambda: (rp.sample(S, seed=1, method="pathwise"),)
    yield "pathwise 48x48 N=600 noiseless", lambda: (rp.sample(S, seed=1, noiseless=True, method="pathwise"),)
    rb = gpim_amd.skreconstructor(Xf, full, Xf, kernel="Matern52", **kw)
    yield "blocks 48x48 (%s)" % rb.solver, lambda: (rb.sample(S, seed=2, method="blocks"),)
    yield "blocks 48x48 noiseless", lambda: (rb.sample(S, seed=2, noiseless=True, method="blocks"),)
    Rm = full.copy()
    for hole in ((3, 4), (9, 2), (20, 31), (40, 7), (47, 47)):
        Rm[hole] = np.nan
    rm = gpim_amd.skreconstructor(gpim_amd.utils.get_sparse_grid(Rm), Rm, Xf, kernel="Matern52", **kw)
    yield "border 48x48 5 missing (%s)" % rm.solver, lambda: (rm.sample(S, seed=3, method="border"),)
    yield "predict border 48x48", lambda: rm.predict(verbose=0)
    # ---- the multi-output model, T = 2
    _, f16 = image((16, 16))
    X16 = gpim_amd.utils.get_full_grid(f16)
    Y = np.stack([f16, np.cos(f16) + 0.1 * image((16, 16), seed=4)[1]], -1)
    for solver, method in (("dense", "joint"), ("reflection", "blocks")):
        rv = gpim_amd.vreconstructor(X16.astype(np.float64), Y, X16, kernel="Matern52", solver=solver, **kw)
        yield "vgp %s T=2 16x16 (%s)" % (method, rv.solver), lambda rv=rv, method=method: (rv.sample(S, seed=4, method=method),)
    # ---- the spectral mixture, Q = 2
    R16, _ = image((16, 16), 200)
    Xs16 = gpim_amd.utils.get_sparse_grid(R16)
    rs = gpim_amd.skreconstructor(Xs16, R16, X16, kernel="Spectral", n_mixtures=2, verbose=0)
    yield "spectral joint Q=2 16x16 N=200", lambda: (rs.sample(S, seed=5, method="joint"),)
    yield "spectral pathwise Q=2 16x16 N=200", lambda: (rs.sample(S, seed=5, method="pathwise"),)
    rsf = gpim_amd.skreconstructor(X16, f16, X16, kernel="Spectral", n_mixtures=2, verbose=0)
    yield "spectral blocks Q=2 16x16 (%s)" % rsf.solver, lambda: (rsf.sample(S, seed=5, method="blocks"),)
    # ---- the dense-by-Kronecker blocks
    Xc, yc = columns_cube()
    rc = gpim_amd.skreconstructor(Xc, yc, None, kernel="RBF", lengthscale=[[0.5] * 3, [20.0] * 3], learning_rate=0.05,
                                  iterations=10, verbose=0)
    rows = np.arange(11) * 4.0 + 0.5
    for name, taxes in (("shared union", (rows, np.arange(6.0), np.arange(5.0))),
                        ("own union", (rows, np.arange(6.0) + 0.25, np.arange(5.0)))):
        Xt = grid(*taxes)
        yield "columns sample, %s (%s)" % (name, rc.solver), lambda Xt=Xt: (rc.sample(S, seed=6, Xtest=Xt, method="columns"),)
        yield "columns predict, %s" % name, lambda Xt=Xt: rc.predict(Xt, verbose=0)
        yield "columns sample S=10 groups of 4, %s" % name, lambda Xt=Xt: with_env(
            "GPIMHIP_PKRON_DRAW_GROUP", "4", lambda: (rc.sample(10, seed=6, Xtest=Xt, method="columns"),))
    yield from training_cases("columns (48, 6, 5)", rc)
    # ---- the Kronecker model
    _, fk = image((12, 10))
    Xk = gpim_amd.utils.get_full_grid(fk)
    rk = gpim_amd.reconstructor(Xk, fk, Xk, kernel="RBF", structured=True, learning_rate=0.05, iterations=10, **kw)
    yield "kron sample 12x10", lambda: (rk.sample(S, seed=7, method="kron"),)
    yield "kron predict 12x10", lambda: rk.predict(verbose=0)
    Xh = grid(np.arange(0, 11.25, 0.5), np.arange(0, 9.25, 0.5))
    yield "kron sample 12x10, half-step test grid", lambda: (rk.sample(S, seed=7, Xtest=Xh, method="kron"),)
    yield from training_cases("kron 12x10", rk)
    yield "dist N=700, one device", dist_case
    # ---- prediction and training of the spectral-mixture and the multi-output drivers, three regimes each
    R3, X3 = f16.copy(), X16.astype(np.float64)
    for hole in ((3, 4), (9, 2), (15, 15)):
        R3[hole] = np.nan
        X3[(slice(None),) + hole] = np.nan
    fine = gpim_amd.utils.get_full_grid(f16, dense_x=0.5)
    Z = np.random.default_rng(8).uniform(-1.0, 17.0, size=(70, 2))
    for regime, X, y, solver in (("dense", Xs16, R16, "dense"), ("blocks", X16, f16, None), ("border", X3, R3, None)):
        rec = gpim_amd.skreconstructor(X, y, X16, kernel="Spectral", n_mixtures=2, learning_rate=0.05, iterations=10, verbose=0,
                                       solver=solver)
        if regime != "border":
            yield "sm %s kmat, symmetric and cross" % regime, lambda rec=rec: (sm_kmat(rec, None), sm_kmat(rec, Z))
        yield from model_cases("sm %s Q=2 16x16 (%s)" % (regime, rec.solver), rec, ("weights", "means", "scales", "noise"),
                               fine if regime != "blocks" else None)
    Y3 = Y.copy()
    Y3[np.isnan(R3)] = np.nan
    for regime, X, y, solver in (("dense", X16.astype(np.float64), Y, "dense"), ("blocks", X16.astype(np.float64), Y, "reflection"),
                                 ("border", X3, Y3, "border")):
        rec = gpim_amd.vreconstructor(X, y, X16, kernel="Matern52", solver=solver, learning_rate=0.05, iterations=10, **kw)
        if regime == "dense":
            yield "vgp dense T=2 16x16 predict, slab path", lambda rec=rec: slab_predict(rec)
        yield from model_cases("vgp %s T=2 16x16 (%s)" % (regime, rec.solver), rec, ("lengthscale",),
                               fine if regime == "blocks" else None)
    yield "predict N=300 M=340, slab path", lambda: slab_predict(r)
    # ---- the stationary training paths (csrc/grad.hip), leave-one-out, the acquisition sweep and the small-grid ranking
    Rd, _ = image((20, 17), 300)                  # (the data of the first case: N = 300 on a grid of M = 340)
    Xsd, Xfd = sparse_and_full(Rd)
    yield "acquisition EI + top-10, M=340", lambda: acq_topk(r, Xfd, Xsd)
    yield from acquisition_cases(r, Rd, Xfd, Xsd)
    tr = dict(learning_rate=0.05, iterations=10, **kw)
    for kernel, precision in (("RBF", "double"), ("Matern52", "double"), ("RationalQuadratic", "double"), ("RBF", "single")):
        rd = gpim_amd.reconstructor(Xsd, Rd, Xfd, kernel=kernel, precision=precision, **tr)
        if kernel == "Matern52":
            yield "loo dense N=300", lambda rd=rd: loo_arrays(rd)
        yield from training_cases("dense N=300 %s %s" % (kernel, precision), rd)
    rr = gpim_amd.reconstructor(X16, f16, X16, kernel="Matern52", structured=True, **tr)
    yield from training_cases("reflection blocks 16x16 Matern52", rr)
    yield "batch B=3 N=300 T=8", batch_fit


def with_env(name, value, run):
    os.environ[name] = value
    try:
        return run()
    finally:
        del os.environ[name]


def training_cases(name, rec):
    """loss and gradient at the initial parameters, then ten Adam iterations (graph replay); after the model's other cases:
    training moves its parameters"""
    def loss_grad():
        loss, grad = rec.loss_and_grad()
        return np.array([loss]), grad.numpy()
    yield name + " nll_grad", loss_grad

    def train():
        rec.train()
        return [np.array(rec.loss_all), rec._u.cpu().numpy()] + [np.array(rec.hyperparams[k], dtype=np.float64)
                                                                 for k in ("lengthscale", "variance", "noise")]
    yield name + " train T=10", train


def dist_case():
    """gpimhip_dist_begin to a factorisation and a forward / backward solve through DistributedCholesky on one device (the
    smallest order of tests/test_gpu_dist.py): the factor, log det and the solution"""
    import torch
    from gpim_amd.dist_chol import DistributedCholesky
    n = 700
    rng = np.random.default_rng(n)
    B = rng.standard_normal((n, n // 3))
    A = torch.from_numpy(B @ B.T + n * np.eye(n)).cuda()
    ch = DistributedCholesky(n)
    ch.set_from_function(lambda c0, c1: A[:, c0:c1]).factor()
    y = torch.from_numpy(rng.standard_normal(n)).cuda()
    return ch.gather_lower().cpu().numpy(), np.array([ch.logdet()]), ch.solve(y).cpu().numpy()


def loo_arrays(rec):
    mean, sd, score = rec.loo(as_grid=False)
    return mean, sd, np.array([score["elpd"], score["rmse"]])


def acq_topk(rec, Xf, Xs):
    """expected improvement over the grid (predictions, nanmax of the incumbent, the sweep), then the ten largest values by
    gpimhip_topk: M = 340 takes the single-workgroup forms"""
    import torch
    from gpim_amd import _lib, acqfunc
    acq, (mean, sd) = acqfunc.expected_improvement(rec, Xf, Xs)
    H = rec._handle
    xd = torch.as_tensor(np.ascontiguousarray(acq, dtype=np.float64).ravel()).to(H.device)
    vals = torch.empty(10, dtype=torch.float64, device=H.device)
    idx = torch.empty(10, dtype=torch.int64, device=H.device)
    cnt = torch.zeros(1, dtype=torch.int64, device=H.device)
    _lib.check(H.lib.gpimhip_topk(H.h, _lib.ptr(xd), xd.numel(), 10, 0, _lib.ptr(vals), _lib.ptr(idx), _lib.ptr(cnt)))
    return acq, mean, sd, vals.cpu().numpy(), idx.cpu().numpy(), cnt.cpu().numpy()


def acquisition_cases(rec, R, Xf, Xs):
    """The acquisition layer on the N = 300 / M = 340 data (np = 384: the fused launch unless the line says slab path):
    gpimhip_acquire_exact (map, mean, sd) and gpimhip_acq for the three kinds, rec.ivr(), the two batch entries, three
    boptimizer steps per batch mode, and the multi-block ranking forms on a seeded vector of 5000"""
    import torch
    from gpim_amd import _lib, acqfunc
    H = rec._handle
    mask = np.where(np.random.default_rng(11).uniform(size=R.shape) < 0.2, np.nan, 1.0)
    params = {"cb": (0.3, 1.5), "ei": (0.0, 0.0), "poi": (0.0, 0.0)}

    def exact(kind, masked):
        mask_d = torch.from_numpy(mask.ravel().copy()).to(H.device) if masked else None
        return [t.cpu().numpy() for t in acqfunc.acquisition_on_device(rec, kind, Xf, Xs, *params[kind], xi=0.01, mask_d=mask_d)]
    for kind in ("cb", "ei", "poi"):
        for masked in (False, True):
            name = "acquire_exact %s%s" % (kind, ", mask" if masked else "")
            yield name, lambda kind=kind, masked=masked: exact(kind, masked)
            yield name + ", slab path", lambda kind=kind, masked=masked: with_env(
                "GPIMHIP_NO_FUSED_PREDICT", "1", lambda: exact(kind, masked))

    def sweep(kind):
        mean, sd = rec.predict(verbose=0)
        md, sdd = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).ravel()).to(H.device) for a in (mean, sd))
        p0, p1 = (0.3, 1.5) if kind == "cb" else (float(np.nanmax(mean)) - 0.1, 0.01)
        return (acqfunc._sweep(H, kind, md, sdd, p0, p1, mean.shape)[0],)
    for kind in ("cb", "ei", "poi"):
        yield "gpimhip_acq %s" % kind, lambda kind=kind: sweep(kind)

    def batch(out):
        points, values, maps = out
        return [np.array(points), values] + [maps[k] for k in sorted(maps)]
    # (Xf again: the expected-improvement case above has left the rows of Xs, NaN included, as the stored test grid)
    yield "rec.ivr()", lambda: rec.ivr(Xf)
    yield "rec.ivr_batch(4)", lambda: batch(rec.ivr_batch(4, Xf))
    for kind in ("cb", "ei", "poi"):
        yield "rec.acq_batch(4, %s)" % kind, lambda kind=kind: batch(rec.acq_batch(4, kind, Xf, alpha=0.3, beta=1.5, mask=mask))

    def campaign(af, **kw):
        import tempfile
        full = image(R.shape)[1]
        np.random.seed(0)                           # (update_points pads a thinned batch from np.random)
        bo = gpim_amd.boptimizer(Xs, R.copy(), Xf, lambda idx: full[tuple(idx)], acquisition_function=af, exploration_steps=3,
                                 batch_size=50, batch_update=True, kernel="Matern52", lengthscale=LS2, gp_iterations=10,
                                 batch_out_max=4, verbose=0, filename=os.path.join(tempfile.mkdtemp(), "bo"), **kw)
        bo.run()
        return np.array(bo.indices_all), np.array(bo.vals_all)
    yield "boptimizer ei, 3 steps, thinned batch", lambda: campaign("ei")
    yield "boptimizer ivr, 3 steps, ivr_batch=greedy", lambda: campaign("ivr", ivr_batch="greedy")
    yield "boptimizer ei, 3 steps, acq_batch=believer", lambda: campaign("ei", acq_batch="believer")

    def rank():
        x = np.random.default_rng(12).standard_normal(5000)
        x[::97] = np.nan
        xd = torch.from_numpy(x).to(H.device)
        vals = torch.empty(10, dtype=torch.float64, device=H.device)
        idx = torch.empty(10, dtype=torch.int64, device=H.device)
        cnt = torch.zeros(1, dtype=torch.int64, device=H.device)
        best = torch.empty(1, dtype=torch.float64, device=H.device)
        _lib.check(H.lib.gpimhip_topk(H.h, _lib.ptr(xd), 5000, 10, 0, _lib.ptr(vals), _lib.ptr(idx), _lib.ptr(cnt)))
        _lib.check(H.lib.gpimhip_nanmax(H.h, _lib.ptr(xd), 5000, _lib.ptr(best)))
        return [t.cpu().numpy() for t in (vals, idx, cnt, best)]
    yield "topk M=5000 k=10 (radix), nanmax n=5000 (two-stage)", rank


def batch_fit():
    """three data sets of N = 300 on a 35 x 35 grid fitted in lock-step (8 iterations: graph replay) and predicted"""
    from gpim_amd.batch import fit_predict_batch
    images = [image((35, 35), 300, seed)[0] for seed in (1, 2, 3)]
    out = fit_predict_batch([gpim_amd.utils.get_sparse_grid(R) for R in images], images, gpim_amd.utils.get_full_grid(images[0]),
                            kernel="Matern52", lengthscale=LS2, learning_rate=0.1, iterations=8)
    return [t.cpu().numpy() for t in out]


def slab_predict(rec):
    """predict() through the chunk loop at a size where the stationary dense model would take the fused launch"""
    return with_env("GPIMHIP_NO_FUSED_PREDICT", "1", lambda: rec.predict(verbose=0))


def model_cases(name, rec, hyper, fine):
    """predict (at the stored test grid and, where given, at the M = 961 points of `fine`: several column tiles in the default
    chunk), loss and gradient, then ten Adam iterations (graph replay): losses, history and final raw parameters"""
    yield name + " predict", lambda: rec.predict(verbose=0)
    if fine is not None:
        yield name + " predict M=961", lambda: rec.predict(fine, verbose=0)
    yield name + " nll_grad", lambda: rec.nll_grad()

    def train():
        rec.train()
        return [np.array(rec.loss_all), rec._u.cpu().numpy()] + [np.array(rec.hyperparams[k], dtype=np.float64) for k in hyper]
    yield name + " train T=10", train


def sm_kmat(rec, Z):
    """gpimhip_sm_kmat at the model's raw parameters: K(X, X) (Z None) or K(X, Z); in reflection mode the stacked blocks"""
    import contextlib
    import ctypes
    import torch
    from gpim_amd import _lib
    blocks = rec.solver != "dense"
    with (rec._solver._mode(rec) if blocks else contextlib.nullcontext()) as D:
        X = D.Xq if blocks else rec._Xd
        N, B = X.shape[0], D.B if blocks else 1
        M = N if Z is None else Z.shape[0]
        Zd = None if Z is None else torch.as_tensor(Z, dtype=torch.float64, device=rec._dev).contiguous()
        out = torch.zeros((B * N, M), dtype=torch.float64, device=rec._dev)
        _lib.check(rec._handle.lib.gpimhip_sm_kmat(rec._handle.h, ctypes.byref(rec._sstruct), _lib.ptr(X), N,
                                                   None if Zd is None else _lib.ptr(Zd), M, _lib.ptr(rec._u), _lib.ptr(out), M))
        return out.cpu().numpy()


def main():
    for name, run in cases():
        print("%-44s %s" % (name, sha(*run())), flush=True)


if __name__ == "__main__":
    main()
