"""
Pathwise posterior draws on the MI355X: gpimhip_sample_pathwise, reconstructor.sample(
method='pathwise') and boptimizer(acquisition_function='ts', ts_method='pathwise') against the host oracle of
tests/pathwise_oracle.py on the same standard normals -- device and oracle are both pure functions of z.

Bar of the draws: 10 x the host discrepancy recorded by tests/test_pathwise_host.py (pathwise_oracle.HOST_DISCREPANCY, the
rounding level of the recipe in float64) x the condition number reported for the case (the largest among K + s I and the
prior blocks K_b + d I: the draws are forward quantities of their Cholesky factors).  The margin of 10 is for the different
summation order and the blocked factors.  The mean is held to predict()'s at the bar of tests/test_gpu_sample.py (1e-10).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
from numpy.testing import assert_allclose

pytestmark = pytest.mark.gpu

import pathwise_oracle as PO
import sample_oracle as SO

ATOL_MEAN = 1e-10


@pytest.fixture(scope="module")
def eng(ensure_built):
    from gpim_amd import _lib
    H = _lib.Handle()
    yield _lib, H
    H.close()


def dev(t):
    return (torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t).cuda().contiguous()


@functools.lru_cache(maxsize=None)
def blocks_of(shape):
    return PO.Blocks(PO.full_grid(shape)[0])


@functools.lru_cache(maxsize=None)
def problem(shape, N, kind, ard):
    """One model on one grid, built once: parameters held identically by the oracle and the engine, N training points
    of the grid in random order, observations, the oracle's blocks and the case's condition number."""
    d = len(shape)
    ls = [[1.0] * d, [6.0] * d] if ard else [1.0, 6.0]
    kp, spec, u = SO.pair(kind, d, ls, seed=3)
    P = PO.Params.from_oracle(kp, d, SO.JITTER)
    blocks = blocks_of(shape)
    idx = np.random.default_rng(N).permutation(blocks.M)[:N].astype(np.int64)
    X = blocks.G[idx]
    y = np.sin(X.sum(1) / 5.0) + 0.1 * np.random.default_rng(N + 1).standard_normal(N)
    return dict(P=P, spec=spec, u=u, blocks=blocks, idx=idx, y=y, cond=PO.condition(P, blocks, idx), shape=shape)


def pathwise_call(_lib, H, Q, Z, noiseless, jitter=SO.JITTER, want_mean=True):
    """gpimhip_sample_pathwise -> (samples (S, M), mean or None) on the host"""
    blocks, spec = Q["blocks"], Q["spec"]
    m = spec.struct()
    S, M, N = Z.shape[0], blocks.M, len(Q["idx"])
    Gd, idxd, yd, ud, Zd = dev(blocks.G), dev(Q["idx"]), dev(Q["y"]), dev(Q["u"]), dev(Z)
    out = torch.full((S, M), float("nan"), dtype=torch.float64, device="cuda")
    mean = torch.full((M,), float("nan"), dtype=torch.float64, device="cuda") if want_mean else None
    shape = (ctypes.c_int32 * len(Q["shape"]))(*Q["shape"])
    mask = sum(1 << k for k in blocks.dims)
    twoc = (ctypes.c_double * 4)(*(list(blocks.S["twoc"])))
    _lib.check(H.lib.gpimhip_sample_pathwise(H.h, ctypes.byref(m), _lib.ptr(Gd), shape, mask, twoc,
                                             ctypes.c_void_p(idxd.data_ptr()), _lib.ptr(yd), N, _lib.ptr(ud), _lib.ptr(Zd), S,
                                             int(noiseless), float(jitter), _lib.ptr(mean), _lib.ptr(out)))
    return out.cpu().numpy(), (mean.cpu().numpy() if want_mean else None)


# 6x5: one odd axis (a mirror plane and weights); 24x24: the fundamental domain has 144 points (crosses a 128-block), N = 130
# crosses one too; the 4x3x4 cube with an isotropic and an ARD lengthscale
CASES = (((6, 5), 1, "RBF", True), ((6, 5), 7, "RBF", True), ((6, 5), 7, "Matern52", True),
         ((6, 5), 7, "RationalQuadratic", True), ((24, 24), 37, "Matern52", True), ((24, 24), 130, "RationalQuadratic", True),
         ((24, 24), 130, "RBF", True), ((4, 3, 4), 9, "RBF", False), ((4, 3, 4), 9, "Matern52", True))


def case_id(c):
    return "%s-N%d-%s-%s" % ("x".join(str(n) for n in c[0]), c[1], c[2], "ard" if c[3] else "iso")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_draws_against_oracle(eng, case):
    _lib, H = eng
    Q = problem(*case)
    blocks, P, idx, y = Q["blocks"], Q["P"], Q["idx"], Q["y"]
    M, N = blocks.M, len(idx)
    tol = 10.0 * PO.HOST_DISCREPANCY * Q["cond"]
    worst = 0.0
    # the posterior mean: gpimhip_predict_exact on the same handle
    m = Q["spec"].struct()
    Xd, yd, ud, Gd = dev(blocks.G[idx]), dev(y), dev(Q["u"]), dev(blocks.G)
    pm = torch.empty(M, dtype=torch.float64, device="cuda")
    pv = torch.empty_like(pm)
    _lib.check(H.lib.gpimhip_predict_exact(H.h, ctypes.byref(m), _lib.ptr(Xd), _lib.ptr(yd), N, _lib.ptr(ud), _lib.ptr(Gd), M,
                                           _lib.ptr(pm), _lib.ptr(pv)))
    for noiseless in (1, 0):
        W = M + N + (0 if noiseless else M)
        Z9 = np.random.default_rng(100 + noiseless).standard_normal((9, W))
        kept = {}
        for S in (9, 3, 1):                                  # 9 spans two groups (8 + 1)
            Z = Z9[4:5] if S == 1 else Z9[:S]
            out, mean = pathwise_call(_lib, H, Q, Z, noiseless)
            ref = PO.draws(P, blocks, idx, y, Z, noiseless)
            err = np.abs(out - ref["out"]).max()
            worst = max(worst, err)
            print("%s noiseless=%d S=%d: draws - oracle %.3e (bar %.3e, cond %.3e), mean - predict %.3e, mean - oracle %.3e"
                  % (case_id(case), noiseless, S, err, tol, Q["cond"], np.abs(mean - pm.cpu().numpy()).max(),
                     np.abs(mean - ref["mean"]).max()))
            assert np.isfinite(out).all()
            assert_allclose(out, ref["out"], rtol=0, atol=tol)
            assert_allclose(mean, pm.cpu().numpy(), rtol=0, atol=ATOL_MEAN)
            assert_allclose(mean, ref["mean"], rtol=0, atol=ATOL_MEAN)
            kept[S] = out
        # a draw's bits do not depend on S or on the group it falls into
        assert np.array_equal(kept[1][0], kept[9][4])
        assert np.array_equal(kept[3], kept[9][:3])
        # null mean output: the same draws, bit for bit
        out0, _ = pathwise_call(_lib, H, Q, Z9[:3], noiseless, want_mean=False)
        assert np.array_equal(out0, kept[3])
    print("%s: worst draws - oracle %.3e" % (case_id(case), worst))


def test_draws_beyond_one_panel(eng):
    """The orders the feature exists for, at their smallest: a 64 x 64 grid (prior blocks of 1024 points: the padded leading
    dimension np + 16, four 256-column chunks of the sweeps L_b z_p) with N = 1100 training points (np = 1152: nine
    128-blocks, three outer panels of the vector solves, so the row sweeps below a panel, the transposed products of the
    backward pass and the inverted diagonal blocks past the first panel all run; the padded leading dimension again).
    Same oracle, same bar as test_draws_against_oracle; the dense host factors of order 4096 take seconds."""
    _lib, H = eng
    shape, N, S = (64, 64), 1100, 3
    kp, spec, u = SO.pair("Matern52", 2, [[1.0, 1.0], [6.0, 6.0]], seed=3)
    P = PO.Params.from_oracle(kp, 2, SO.JITTER)
    blocks = PO.Blocks(PO.full_grid(shape)[0])                # (not cached: its basis change holds 128 MiB)
    M = blocks.M
    assert blocks.Nq == 1024 and blocks.B == 4
    idx = np.random.default_rng(N).permutation(M)[:N].astype(np.int64)
    X = blocks.G[idx]
    y = np.sin(X.sum(1) / 5.0) + 0.1 * np.random.default_rng(N + 1).standard_normal(N)
    cond = PO.condition(P, blocks, idx)
    Q = dict(P=P, spec=spec, u=u, blocks=blocks, idx=idx, y=y, cond=cond, shape=shape)
    tol = 10.0 * PO.HOST_DISCREPANCY * cond
    m = spec.struct()
    Xd, yd, ud, Gd = dev(X), dev(y), dev(u), dev(blocks.G)
    pm = torch.empty(M, dtype=torch.float64, device="cuda")
    pv = torch.empty_like(pm)
    _lib.check(H.lib.gpimhip_predict_exact(H.h, ctypes.byref(m), _lib.ptr(Xd), _lib.ptr(yd), N, _lib.ptr(ud), _lib.ptr(Gd), M,
                                           _lib.ptr(pm), _lib.ptr(pv)))
    Z = np.random.default_rng(7).standard_normal((S, 2 * M + N))
    out, mean = pathwise_call(_lib, H, Q, Z, 0)
    ref = PO.draws(P, blocks, idx, y, Z, False)
    print("64x64-N1100-Matern52-ard S=3: draws - oracle %.3e (bar %.3e, cond %.3e), mean - predict %.3e, mean - oracle %.3e"
          % (np.abs(out - ref["out"]).max(), tol, cond, np.abs(mean - pm.cpu().numpy()).max(),
             np.abs(mean - ref["mean"]).max()))
    assert np.isfinite(out).all()
    assert_allclose(out, ref["out"], rtol=0, atol=tol)
    assert_allclose(mean, pm.cpu().numpy(), rtol=0, atol=ATOL_MEAN)
    assert_allclose(mean, ref["mean"], rtol=0, atol=ATOL_MEAN)
    # a draw's bits do not depend on S at these orders either
    one, _ = pathwise_call(_lib, H, Q, Z[1:2], 0, want_mean=False)
    assert np.array_equal(one[0], out[1])


def test_joint_against_pathwise_8x8(eng):
    """The covariance of p from identity probes against the joint route's L22 L22^T: they differ by the terms that carry d,
    max |Sigma_pw - Sigma| <= COV_SHIFT_OVER_D d (tests/test_pathwise_host.py); twice that is the bar."""
    _lib, H = eng
    Q = problem((8, 8), 11, "Matern52", True)
    blocks, idx = Q["blocks"], Q["idx"]
    M, N = blocks.M, len(idx)
    Q0 = dict(Q, y=np.zeros(N))
    out, mean = pathwise_call(_lib, H, Q0, np.eye(M + N), 1)
    A = (out - mean[None, :]).T                             # p = A z
    cov_pw = A @ A.T
    m = Q["spec"].struct()
    Xd, yd, ud, Gd = dev(blocks.G[idx]), dev(Q["y"]), dev(Q["u"]), dev(blocks.G)
    Zd = torch.eye(M, dtype=torch.float64, device="cuda")
    smp = torch.empty((M, M), dtype=torch.float64, device="cuda")
    jm = torch.empty(M, dtype=torch.float64, device="cuda")
    _lib.check(H.lib.gpimhip_sample_exact(H.h, ctypes.byref(m), _lib.ptr(Xd), _lib.ptr(yd), N, _lib.ptr(ud), _lib.ptr(Gd), M,
                                          _lib.ptr(Zd), M, 1, SO.JITTER, _lib.ptr(jm), None, _lib.ptr(smp)))
    D = (smp - jm[None, :]).t().cpu().numpy()
    diff = np.abs(cov_pw - D @ D.T).max()
    bar = PO.COV_SHIFT_OVER_D * SO.JITTER * 2.0
    print("8x8: |cov(p) - L22 L22^T| %.3e (bar %.3e); cov(p) - Sigma_pw (oracle) %.3e"
          % (diff, bar, np.abs(cov_pw - PO.sigma_pathwise(Q["P"], blocks, idx)).max()))
    assert diff <= bar
    assert diff > 0.01 * SO.JITTER                          # and they do differ: the jittered process is another process


def test_bad_arguments_and_workspace(eng):
    _lib, H = eng
    Q = problem((6, 5), 7, "RBF", True)
    blocks = Q["blocks"]
    M, N = blocks.M, 7
    Z = np.zeros((1, M + N))
    bytes0 = H.lib.gpimhip_workspace_bytes(H.h)
    a, _ = pathwise_call(_lib, H, Q, Z, 1)
    bytes1 = H.lib.gpimhip_workspace_bytes(H.h)
    b, _ = pathwise_call(_lib, H, Q, Z, 1)
    assert H.lib.gpimhip_workspace_bytes(H.h) == bytes1 and bytes1 >= bytes0 and np.array_equal(a, b)
    for bad in (0.0, -1e-9, float("nan")):
        with pytest.raises(ValueError):
            pathwise_call(_lib, H, Q, Z, 1, jitter=bad)
    # no reflected axis, an axis bit beyond the dimension, a single-precision handle
    m = Q["spec"].struct()
    Gd, idxd, yd, ud, Zd = dev(blocks.G), dev(Q["idx"]), dev(Q["y"]), dev(Q["u"]), dev(Z)
    out = torch.empty((1, M), dtype=torch.float64, device="cuda")
    shape, twoc = (ctypes.c_int32 * 2)(6, 5), (ctypes.c_double * 4)(5.0, 4.0, 0.0, 0.0)

    def rc(h=H, mask=3, S=1, idx=idxd, o=out):
        return h.lib.gpimhip_sample_pathwise(h.h, ctypes.byref(m), _lib.ptr(Gd), shape, mask, twoc,
                                             None if idx is None else ctypes.c_void_p(idx.data_ptr()), _lib.ptr(yd), N,
                                             _lib.ptr(ud), _lib.ptr(Zd), S, 1, 1e-5, None, _lib.ptr(o))
    assert rc() == _lib.OK
    for kw in (dict(mask=0), dict(mask=4), dict(S=0), dict(idx=None), dict(o=None)):
        assert rc(**kw) == _lib.E_BADARG, kw
    H32 = _lib.Handle(precision="single")
    try:
        assert rc(h=H32) == _lib.E_BADARG
    finally:
        H32.close()


# ------------------------------------------------------------------------------------------ Python surface
def image16(seed=0, n_obs=60):
    rng = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    R = np.sin(ii / 3.0) * np.cos(jj / 4.0) + 0.05 * rng.standard_normal((16, 16))
    full = R.copy()
    R.ravel()[rng.permutation(256)[n_obs:]] = np.nan
    return R, full


@pytest.fixture(scope="module")
def fitted(ensure_built):
    import gpim_amd
    R, _ = image16()
    r = gpim_amd.reconstructor(gpim_amd.utils.get_sparse_grid(R), R, gpim_amd.utils.get_full_grid(R), kernel="Matern52",
                               lengthscale=[[1., 1.], [8., 8.]], learning_rate=0.1, iterations=20, verbose=0)
    r.train()
    return gpim_amd, r, R


def oracle_params(r):
    var, ls, noise = r._spec.constrained(r._u)
    d = r._spec.dim
    alpha = float(torch.exp(r._u[2 + r._spec.n_ls])) if r._spec.kernel_type == "RationalQuadratic" else 1.0
    return PO.Params(r._spec.kernel_type, float(var), np.broadcast_to(ls.numpy().reshape(-1), (d,)).copy(), float(noise), alpha,
                     r._spec.jitter)


def oracle_for(r, shape):
    """(Params, Blocks, idx, y) of a dense reconstructor whose test grid is the index grid of `shape`"""
    from gpim_amd import gprutils
    blocks = blocks_of(tuple(shape))
    X = r._Xd.cpu().numpy()
    idx = gprutils.pathwise_grid(PO.full_grid(tuple(shape))[0], X)["idx"]
    return oracle_params(r), blocks, idx, r._yd.cpu().numpy()


def test_reconstructor_sample_pathwise(fitted):
    gpim_amd, r, R = fitted
    M, N = 256, r._Xd.shape[0]
    P, blocks, idx, y = oracle_for(r, (16, 16))
    tol = 10.0 * PO.HOST_DISCREPANCY * PO.condition(P, blocks, idx)
    a = r.sample(n_samples=3, seed=1, method="pathwise")
    assert a.shape == (3, 16, 16) and a.dtype == np.float64 and np.isfinite(a).all()
    assert np.array_equal(a, r.sample(n_samples=3, seed=1, method="pathwise"))
    assert not np.array_equal(a, r.sample(n_samples=3, seed=2, method="pathwise"))
    assert r.sample(method="pathwise").shape == (1, 16, 16)
    # the documented rule for the implicit draw, at the pathwise width
    for noiseless in (False, True):
        W = M + N + (0 if noiseless else M)
        z = torch.randn((3, W), dtype=torch.float64, device=r._dev, generator=torch.Generator(r._dev).manual_seed(1))
        got = r.sample(n_samples=3, z=z, noiseless=noiseless, method="pathwise")
        assert np.array_equal(got, r.sample(n_samples=3, seed=1, noiseless=noiseless, method="pathwise"))
        assert np.array_equal(got, r.sample(n_samples=3, z=z.cpu().numpy(), noiseless=noiseless, method="pathwise"))
        ref = PO.draws(P, blocks, idx, y, z.cpu().numpy(), noiseless)["out"].reshape(3, 16, 16)
        print("reconstructor.sample(pathwise) noiseless=%d: draws - oracle %.3e (bar %.3e)"
              % (noiseless, np.abs(got - ref).max(), tol))
        assert_allclose(got, ref, rtol=0, atol=tol)
    with pytest.raises(ValueError):
        r.sample(n_samples=2, z=z, method="pathwise")
    with pytest.raises(ValueError):
        r.sample(n_samples=3, z=z[:, :M], noiseless=True, method="pathwise")        # the joint route's width
    with pytest.raises(ValueError):
        r.sample(method="matheron")
    # the default is the joint route, untouched
    zj = torch.randn((2, M), dtype=torch.float64, device=r._dev, generator=torch.Generator(r._dev).manual_seed(7))
    assert np.array_equal(r.sample(n_samples=2, z=zj), r.sample(n_samples=2, z=zj, method="joint"))


def test_errors(fitted):
    gpim_amd, r, R = fitted
    from gpim_amd import _lib
    Xs, Xf = gpim_amd.utils.get_sparse_grid(R), gpim_amd.utils.get_full_grid(R)
    before = r.sample(n_samples=1, seed=4, method="pathwise")
    # d > s and d <= 0
    for bad in (10.0, 0.0, -1e-6):
        with pytest.raises(ValueError):
            r.sample(method="pathwise", jitter=bad)
    # a NaN grid (refused before it replaces the stored one)
    Xnan = Xf.astype(np.float64)
    Xnan[:, 3, 4] = np.nan
    with pytest.raises(ValueError):
        r.sample(Xtest=Xnan, method="pathwise")
    assert np.array_equal(before, r.sample(n_samples=1, seed=4, method="pathwise"))
    # a training row off the grid: the same grid moved by half a pixel
    with pytest.raises(NotImplementedError, match="not on it"):
        r.sample(Xtest=Xf + 0.5, method="pathwise")
    # a grid without a symmetric axis
    ax = np.concatenate([np.arange(15.0), [20.0]])
    Xu = np.array(np.meshgrid(ax, ax, indexing="ij"))
    with pytest.raises(NotImplementedError, match="symmetric"):
        r.sample(Xtest=Xu, method="pathwise")
    # test rows that are no grid at all
    with pytest.raises(NotImplementedError, match="product grid"):
        r.sample(Xtest=Xf.reshape(2, -1), method="pathwise")
    # every refused grid left the stored one in place
    assert r.fulldims == (16, 16) and np.array_equal(before, r.sample(n_samples=1, seed=4, method="pathwise"))
    # each of the other solvers
    _, full = image16()
    models = [gpim_amd.reconstructor(Xs, R, Xf, sparse=True, indpoints=20, iterations=1, verbose=0),
              gpim_amd.reconstructor(Xf, full, Xf, structured=True, iterations=1, verbose=0),
              gpim_amd.reconstructor(Xf, full, Xf, kernel="Matern52", structured=True, iterations=1, verbose=0),
              gpim_amd.reconstructor(Xs, R, Xf, precision="single", iterations=1, verbose=0)]
    for model in models:
        with pytest.raises(NotImplementedError, match="dense double-precision engine"):
            model.sample(method="pathwise")


def test_not_pd_prior_block(fitted):
    """RBF with a lengthscale 20 x the grid and jitter 1e-30: the prior blocks are numerically singular.  numpy's Cholesky
    fails on them too; the library reports it and the reconstructor stays usable."""
    gpim_amd, _, R = fitted
    from gpim_amd import _lib
    Xs, Xf = gpim_amd.utils.get_sparse_grid(R), gpim_amd.utils.get_full_grid(R)
    r = gpim_amd.reconstructor(Xs, R, Xf, kernel="RBF", lengthscale=[[320., 320.], [321., 321.]], jitter=1e-30, iterations=1,
                               verbose=0)
    P, blocks, idx, y = oracle_for(r, (16, 16))
    with pytest.raises(np.linalg.LinAlgError):
        for Kb in blocks.prior_blocks(P, 1e-30):
            np.linalg.cholesky(Kb)
    with pytest.raises(_lib.NotPositiveDefiniteError):
        r.sample(method="pathwise")
    ok = r.sample(n_samples=2, seed=0, method="pathwise", jitter=1e-3)
    assert ok.shape == (2, 16, 16) and np.isfinite(ok).all()
    mean, sd = r.predict(verbose=0)
    assert np.isfinite(mean).all() and np.isfinite(sd).all()


# ------------------------------------------------------------------------------------------ boptimizer
def make_bo(gpim_amd, tmp_path, **kw):
    from problems import bo_test_problem
    f, Z = bo_test_problem()
    return gpim_amd.boptimizer(gpim_amd.utils.get_sparse_grid(Z), Z.copy(), gpim_amd.utils.get_full_grid(Z), f,
                               acquisition_function="ts", exploration_steps=3, gp_iterations=20, learning_rate=0.1, seed=3,
                               verbose=0, filename=str(tmp_path / "bo"), **kw)


def test_boptimizer_thompson_pathwise(fitted, tmp_path):
    gpim_amd = fitted[0]
    runs = []
    for _ in range(2):
        bo = make_bo(gpim_amd, tmp_path, ts_method="pathwise")
        bo.run()
        runs.append(bo)
    a, b = runs
    assert len(a.indices_all) == 3 and a.indices_all == b.indices_all
    assert len(a.gp_predictions) == 3
    # a third optimiser, driven as single_step drives it: before each ranking the host oracle replays the draw with the same
    # z (the generator's stream at the widths M + N of the steps) and ranks it as checkvalues does
    c = make_bo(gpim_amd, tmp_path, ts_method="pathwise")
    sm = c.surrogate_model
    gen = torch.Generator(sm._dev).manual_seed(3)
    M = 625
    for e in range(3):
        if e == 0:
            sm.train()
        N = sm._Xd.shape[0]
        z = torch.randn((1, M + N), dtype=torch.float64, device=sm._dev, generator=gen)
        P, blocks, idx, y = oracle_for(sm, (25, 25))
        draw = PO.draws(P, blocks, idx, y, z.cpu().numpy(), True)["out"][0]
        ranked = [[int(v) for v in np.unravel_index(i, (25, 25))] for i in np.argsort(-draw)[:100]]
        expect = [p for p in ranked if p not in c.indices_all][0]
        if e == 0:
            # the public acquisition function: the same draw; mean and sd from the ordinary prediction
            acq, (mean, sd) = gpim_amd.acqfunc.thompson_sampling(sm, c.X_full, z=z, method="pathwise")
            tol = 10.0 * PO.HOST_DISCREPANCY * PO.condition(P, blocks, idx)
            print("boptimizer step 0: draw - oracle %.3e (bar %.3e)" % (np.abs(acq.reshape(-1) - draw).max(), tol))
            assert_allclose(acq.reshape(-1), draw, rtol=0, atol=tol)
            pm, psd = sm.predict(verbose=0)
            assert_allclose(mean, pm, rtol=0, atol=ATOL_MEAN)
            assert_allclose(sd, psd, rtol=0, atol=ATOL_MEAN)
        vals, inds = c.next_point()
        ind, val = c.checkvalues(inds, vals)
        assert list(ind) == expect, (e, ind, expect)
        c.evaluate_function(ind)
        c.update_posterior()
        c.indices_all.append(ind)
        c.vals_all.append(val)
    assert c.indices_all == a.indices_all


def test_boptimizer_batch_of_draws(fitted, tmp_path):
    gpim_amd = fitted[0]
    bo = make_bo(gpim_amd, tmp_path, ts_method="pathwise", ts_batch="draws", batch_update=True, batch_size=4, batch_out_max=4,
                 batch_dscale=0)
    bo.surrogate_model.train()
    vals, inds = bo.next_point()
    assert len(inds) == 4 and len({tuple(i) for i in inds}) == 4 and len(vals) == 4
    assert vals == sorted(vals, reverse=True)
    # the default keeps a single draw's top-k
    bo1 = make_bo(gpim_amd, tmp_path, ts_method="pathwise", batch_update=True, batch_size=4, batch_out_max=4, batch_dscale=0)
    assert bo1.ts_batch == "topk"
    with pytest.raises(ValueError):
        make_bo(gpim_amd, tmp_path, ts_batch="all")
    with pytest.raises(ValueError):
        make_bo(gpim_amd, tmp_path, ts_method="exact")
    # the joint route takes a batch of draws too
    boj = make_bo(gpim_amd, tmp_path, ts_batch="draws", batch_update=True, batch_size=3, batch_out_max=3, batch_dscale=0)
    boj.surrogate_model.train()
    _, indj = boj.next_point()
    assert len({tuple(i) for i in indj}) == 3
