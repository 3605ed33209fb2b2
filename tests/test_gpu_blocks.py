"""
Posterior draws on a fully observed grid through its reflection blocks on the MI355X:
gpimhip_sample_blocks and reconstructor.sample(method='blocks') against the host oracle of tests/pathwise_oracle.py with
idx = arange(M) on the same standard normals -- device and oracle are both pure functions of z.

Bar of the draws, as in tests/test_gpu_pathwise.py: 10 x pathwise_oracle.HOST_DISCREPANCY (the rounding level of the recipe in
float64) x the condition number of the case (the largest among K + s I and the prior blocks K_b + d I).  The mean is held to
gpimhip_predict_exact on the same data at 1e-10, the bar of tests/test_gpu_sample.py.
"""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch
from numpy.testing import assert_allclose

pytestmark = pytest.mark.gpu

import pathwise_oracle as PO
import sample_oracle as SO

ATOL_MEAN = 1e-10
EPS = np.finfo(np.float64).eps


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


def block_condition(P, blocks, d):
    """pathwise_oracle.condition(P, blocks, arange(M)) without an eigenvalue problem of order M: K + s I is orthogonally
    similar to blockdiag(K_b + s I) on the rows that exist, so its extreme eigenvalues are the extremes over the blocks."""
    lo, hi, cb = np.inf, 0.0, 0.0
    for b, Kb in enumerate(blocks.prior_blocks(P, d)):
        pr = blocks.present[b]
        w = np.linalg.eigvalsh(Kb[np.ix_(pr, pr)])
        cb = max(cb, float(w[-1] / w[0]))
        lo, hi = min(lo, float(w[0]) + (P.s - d)), max(hi, float(w[-1]) + (P.s - d))
    return max(hi / lo, cb)


@functools.lru_cache(maxsize=None)
def problem(shape, kind, ard=True):
    """One fully observed grid and one model, built once: parameters held identically by the oracle and the engine,
    observations in grid order, the oracle's blocks and the case's condition number."""
    d = len(shape)
    ls = [[1.0] * d, [6.0] * d] if ard else [1.0, 6.0]
    kp, spec, u = SO.pair(kind, d, ls, seed=3)
    P = PO.Params.from_oracle(kp, d, SO.JITTER)
    blocks = blocks_of(shape)
    y = np.sin(blocks.G.sum(1) / 5.0) + 0.1 * np.random.default_rng(blocks.M + 1).standard_normal(blocks.M)
    return dict(P=P, spec=spec, u=u, blocks=blocks, idx=np.arange(blocks.M), y=y, cond=block_condition(P, blocks, SO.JITTER),
                shape=shape)


def blocks_rc(_lib, H, Q, Zd, noiseless, jitter, mean, out, mask=None, S=None, y="y"):
    blocks, spec = Q["blocks"], Q["spec"]
    m = spec.struct()
    Gd, yd, ud = dev(blocks.G), dev(Q["y"]), dev(Q["u"])
    shape = (ctypes.c_int32 * len(Q["shape"]))(*Q["shape"])
    mask = sum(1 << k for k in blocks.dims) if mask is None else mask
    twoc = (ctypes.c_double * 4)(*(list(blocks.S["twoc"])))
    return H.lib.gpimhip_sample_blocks(H.h, ctypes.byref(m), _lib.ptr(Gd), shape, mask, twoc, _lib.ptr(yd) if y else None,
                                       _lib.ptr(ud), _lib.ptr(Zd), Zd.shape[0] if S is None else S, int(noiseless),
                                       float(jitter), _lib.ptr(mean), _lib.ptr(out))


def blocks_call(_lib, H, Q, Z, noiseless, jitter=SO.JITTER, want_mean=True):
    """gpimhip_sample_blocks -> (samples (S, M), mean or None) on the host"""
    S, M = Z.shape[0], Q["blocks"].M
    out = torch.full((S, M), float("nan"), dtype=torch.float64, device="cuda")
    mean = torch.full((M,), float("nan"), dtype=torch.float64, device="cuda") if want_mean else None
    _lib.check(blocks_rc(_lib, H, Q, dev(Z), noiseless, jitter, mean, out))
    return out.cpu().numpy(), (mean.cpu().numpy() if want_mean else None)


def predict_mean(_lib, H, Q):
    blocks = Q["blocks"]
    M = blocks.M
    m = Q["spec"].struct()
    Gd, yd, ud = dev(blocks.G), dev(Q["y"]), dev(Q["u"])
    pm = torch.empty(M, dtype=torch.float64, device="cuda")
    pv = torch.empty_like(pm)
    _lib.check(H.lib.gpimhip_predict_exact(H.h, ctypes.byref(m), _lib.ptr(Gd), _lib.ptr(yd), M, _lib.ptr(ud), _lib.ptr(Gd), M,
                                           _lib.ptr(pm), _lib.ptr(pv)))
    return pm.cpu().numpy()


# 6x5: one odd axis (a mirror plane and weights); 5x5: both odd (a point with a stabiliser of four, blocks of different
# sizes); 4x3x4: eight blocks; 24x24: the fundamental domain has 144 points (crosses a 128-block)
GRIDS = ((6, 5), (5, 5), (4, 3, 4), (24, 24))
CASES = tuple((shape, kind) for shape in GRIDS for kind in SO.KINDS)


def case_id(c):
    return "%s-%s" % ("x".join(str(n) for n in c[0]), c[1])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_draws_against_oracle(eng, case):
    _lib, H = eng
    Q = problem(*case)
    blocks, P = Q["blocks"], Q["P"]
    M = blocks.M
    tol = 10.0 * PO.HOST_DISCREPANCY * Q["cond"]
    pm = predict_mean(_lib, H, Q)
    for noiseless in (1, 0):
        Z = np.random.default_rng(100 + noiseless).standard_normal((3, 2 * M + (0 if noiseless else M)))
        out, mean = blocks_call(_lib, H, Q, Z, noiseless)
        ref = PO.draws(P, blocks, Q["idx"], Q["y"], Z, noiseless)
        print("%s noiseless=%d S=3: draws - oracle %.3e (bar %.3e, cond %.3e), mean - predict %.3e, mean - oracle %.3e"
              % (case_id(case), noiseless, np.abs(out - ref["out"]).max(), tol, Q["cond"], np.abs(mean - pm).max(),
                 np.abs(mean - ref["mean"]).max()))
        assert np.isfinite(out).all()
        assert_allclose(out, ref["out"], rtol=0, atol=tol)
        assert_allclose(mean, pm, rtol=0, atol=ATOL_MEAN)
        assert_allclose(mean, ref["mean"], rtol=0, atol=ATOL_MEAN)
        # null mean output: the same draws, bit for bit
        out0, _ = blocks_call(_lib, H, Q, Z, noiseless, want_mean=False)
        assert np.array_equal(out0, out)


def test_bits_do_not_depend_on_the_group(eng):
    """Draw k of an S = 9 call (columns in groups of 8 and 2, y in the second) is the S = 1 call on the same row of z (one
    group of 2) and the S = 3 call (one group of 4), and the mean does not depend on the group that carries y."""
    _lib, H = eng
    Q = problem((24, 24), "Matern52")
    M = Q["blocks"].M
    for noiseless in (1, 0):
        Z9 = np.random.default_rng(5 + noiseless).standard_normal((9, 2 * M + (0 if noiseless else M)))
        o9, m9 = blocks_call(_lib, H, Q, Z9, noiseless)
        o1, m1 = blocks_call(_lib, H, Q, Z9[4:5], noiseless)
        o3, m3 = blocks_call(_lib, H, Q, Z9[:3], noiseless)
        o6, _ = blocks_call(_lib, H, Q, Z9[:6], noiseless)            # seven columns in the form for eight
        assert np.array_equal(o1[0], o9[4]) and np.array_equal(o3, o9[:3]) and np.array_equal(o6, o9[:6])
        assert np.array_equal(m1, m9) and np.array_equal(m3, m9)


def test_draws_beyond_one_panel(eng):
    """72 x 64: blocks of Nq = 1152 points, np = 1152 (nine 128-blocks, ld = np + 16): three outer panels of the solves with a
    ragged last one (a single block), so the multi-column row sweeps below a panel, the transposed products (two row chunks
    below the first panel) and the inverted diagonal blocks past the first panel all run.  S = 9: ten columns, a group of 8
    and a group of 2 that carries y.  Same oracle, same bar; the dense host factors of order 4608 take seconds."""
    _lib, H = eng
    shape, S = (72, 64), 9
    kp, spec, u = SO.pair("Matern52", 2, [[1.0, 1.0], [6.0, 6.0]], seed=3)
    P = PO.Params.from_oracle(kp, 2, SO.JITTER)
    blocks = PO.Blocks(PO.full_grid(shape)[0])                # (not cached: its basis change holds 160 MiB)
    M = blocks.M
    assert blocks.Nq == 1152 and blocks.B == 4
    y = np.sin(blocks.G.sum(1) / 5.0) + 0.1 * np.random.default_rng(M + 1).standard_normal(M)
    cond = block_condition(P, blocks, SO.JITTER)
    Q = dict(P=P, spec=spec, u=u, blocks=blocks, idx=np.arange(M), y=y, cond=cond, shape=shape)
    tol = 10.0 * PO.HOST_DISCREPANCY * cond
    pm = predict_mean(_lib, H, Q)
    Z = np.random.default_rng(7).standard_normal((S, 3 * M))
    out, mean = blocks_call(_lib, H, Q, Z, 0)
    ref = PO.draws(P, blocks, Q["idx"], y, Z, False)
    print("72x64-Matern52 S=9: draws - oracle %.3e (bar %.3e, cond %.3e), mean - predict %.3e, mean - oracle %.3e"
          % (np.abs(out - ref["out"]).max(), tol, cond, np.abs(mean - pm).max(), np.abs(mean - ref["mean"]).max()))
    assert np.isfinite(out).all()
    assert_allclose(out, ref["out"], rtol=0, atol=tol)
    assert_allclose(mean, pm, rtol=0, atol=ATOL_MEAN)
    assert_allclose(mean, ref["mean"], rtol=0, atol=ATOL_MEAN)
    # a draw's bits do not depend on S or on its group at these orders either
    one, m1 = blocks_call(_lib, H, Q, Z[4:5], 0)
    three, _ = blocks_call(_lib, H, Q, Z[:3], 0)
    assert np.array_equal(one[0], out[4]) and np.array_equal(three, out[:3]) and np.array_equal(m1, mean)


def test_covariance_8x8(eng):
    """The covariance of p from identity probes against Sigma_pw of the oracle with idx = arange(M).  Bar: the one of
    tests/test_pathwise_host.py::test_covariance_identity, 100 eps cond variance, with the condition number of the case (the
    probes pass through the factors of K_b + d I and of K_b + s I); it lies far inside the bar of
    tests/test_gpu_pathwise.py::test_joint_against_pathwise_8x8 (2 COV_SHIFT_OVER_D d), which is asserted as well."""
    _lib, H = eng
    Q = problem((8, 8), "Matern52")
    blocks, P = Q["blocks"], Q["P"]
    M = blocks.M
    Q0 = dict(Q, y=np.zeros(M))
    out, mean = blocks_call(_lib, H, Q0, np.eye(2 * M), 1)
    assert np.abs(mean).max() == 0.0
    A = out.T                                               # p = A z
    err = np.abs(A @ A.T - PO.sigma_pathwise(P, blocks, Q["idx"])).max()
    bar = 100.0 * EPS * Q["cond"] * P.var
    print("8x8: |cov(p) - Sigma_pw| %.3e (bar %.3e, cond %.3e)" % (err, bar, Q["cond"]))
    assert bar <= PO.COV_SHIFT_OVER_D * SO.JITTER * 2.0
    assert err <= bar


def test_bad_arguments_and_workspace(eng):
    _lib, H = eng
    Q = problem((6, 5), "RBF")
    M = Q["blocks"].M
    Z = np.zeros((1, 2 * M))
    bytes0 = H.lib.gpimhip_workspace_bytes(H.h)
    a, _ = blocks_call(_lib, H, Q, Z, 1)
    bytes1 = H.lib.gpimhip_workspace_bytes(H.h)
    b, _ = blocks_call(_lib, H, Q, Z, 1)
    assert H.lib.gpimhip_workspace_bytes(H.h) == bytes1 and bytes1 >= bytes0 and np.array_equal(a, b)
    for bad in (0.0, -1e-9, float("nan")):
        with pytest.raises(ValueError):
            blocks_call(_lib, H, Q, Z, 1, jitter=bad)
    Zd = dev(Z)
    out = torch.empty((1, M), dtype=torch.float64, device="cuda")
    rc = lambda h=H, **kw: blocks_rc(_lib, h, Q, Zd, 1, 1e-5, None, kw.pop("o", out), **kw)
    assert rc() == _lib.OK
    # no reflected axis, an axis bit beyond the dimension, no draws, null pointers
    for kw in (dict(mask=0), dict(mask=4), dict(S=0), dict(y=None), dict(o=None)):
        assert rc(**kw) == _lib.E_BADARG, kw
    # a handle in reflection mode, with the wording of the pathwise entry
    mode = types.SimpleNamespace(mask=3, twoc=(ctypes.c_double * 4)(5.0, 4.0, 0.0, 0.0), wts=None, n_total=M)
    with _lib.reflection(H, mode):
        assert rc() == _lib.E_BADARG
        assert b"gpimhip_sample_blocks: not available in reflection mode" in H.lib.gpimhip_last_error()
    assert rc() == _lib.OK
    H32 = _lib.Handle(precision="single")
    try:
        assert rc(h=H32) == _lib.E_BADARG
    finally:
        H32.close()


# ------------------------------------------------------------------------------------------ Python surface
def image16(seed=0):
    rng = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    return np.sin(ii / 3.0) * np.cos(jj / 4.0) + 0.05 * rng.standard_normal((16, 16))


def oracle_params(r):
    var, ls, noise = r._spec.constrained(r._u)
    d = r._spec.dim
    alpha = float(torch.exp(r._u[2 + r._spec.n_ls])) if r._spec.kernel_type == "RationalQuadratic" else 1.0
    return PO.Params(r._spec.kernel_type, float(var), np.broadcast_to(ls.cpu().numpy().reshape(-1), (d,)).copy(), float(noise),
                     alpha, r._spec.jitter)


@pytest.fixture(scope="module")
def models(ensure_built):
    import gpim_amd
    full = image16()
    Xf = gpim_amd.utils.get_full_grid(full)
    kw = dict(lengthscale=[[1., 1.], [8., 8.]], learning_rate=0.1, iterations=3, verbose=0)
    made = {"reflection": gpim_amd.reconstructor(Xf, full, Xf, kernel="Matern52", structured=True, **kw),
            "kronecker": gpim_amd.reconstructor(Xf, full, Xf, kernel="RBF", structured=True, **kw),
            "skreconstructor": gpim_amd.skreconstructor(Xf, full, Xf, kernel="Matern52", **kw),
            "dense": gpim_amd.reconstructor(Xf, full, Xf, kernel="Matern52", **kw)}
    assert made["reflection"].do_symm and made["kronecker"].do_structured and made["skreconstructor"].solver == "reflection"
    for r in made.values():
        r.train()
    return gpim_amd, made, full, Xf


@pytest.mark.parametrize("name", ("reflection", "kronecker", "skreconstructor", "dense"))
def test_reconstructor_sample_blocks(models, name):
    gpim_amd, made, full, Xf = models
    r = made[name]
    M = 256
    P, blocks = oracle_params(r), blocks_of((16, 16))
    idx, y = np.arange(M), full.reshape(-1)
    tol = 10.0 * PO.HOST_DISCREPANCY * block_condition(P, blocks, P.jitter)
    a = r.sample(n_samples=3, seed=1, method="blocks")
    assert a.shape == (3, 16, 16) and a.dtype == np.float64 and np.isfinite(a).all()
    assert np.array_equal(a, r.sample(n_samples=3, seed=1, method="blocks"))
    assert not np.array_equal(a, r.sample(n_samples=3, seed=2, method="blocks"))
    assert r.sample(method="blocks").shape == (1, 16, 16)
    assert np.array_equal(a, r.sample(n_samples=3, seed=1, Xtest=Xf, method="blocks"))      # the training grid, given
    for noiseless in (False, True):
        W = 2 * M + (0 if noiseless else M)
        z = torch.randn((3, W), dtype=torch.float64, device=r._dev, generator=torch.Generator(r._dev).manual_seed(1))
        got = r.sample(n_samples=3, z=z, noiseless=noiseless, method="blocks")
        assert np.array_equal(got, r.sample(n_samples=3, seed=1, noiseless=noiseless, method="blocks"))
        assert np.array_equal(got, r.sample(n_samples=3, z=z.cpu().numpy(), noiseless=noiseless, method="blocks"))
        ref = PO.draws(P, blocks, idx, y, z.cpu().numpy(), noiseless)["out"].reshape(3, 16, 16)
        print("%s.sample(blocks) noiseless=%d: draws - oracle %.3e (bar %.3e)" % (name, noiseless, np.abs(got - ref).max(), tol))
        assert_allclose(got, ref, rtol=0, atol=tol)
        if name == "dense":
            # the same model's pathwise route on the same z: N = M and the rows in grid order, so the layouts coincide
            pw = r.sample(n_samples=3, z=z, noiseless=noiseless, method="pathwise")
            print("dense: blocks - pathwise %.3e (bar %.3e)" % (np.abs(got - pw).max(), 2.0 * tol))
            assert_allclose(got, pw, rtol=0, atol=2.0 * tol)
    # the model still trains and predicts
    mean, sd = r.predict(verbose=0)
    assert mean.shape == (16, 16) and np.isfinite(mean).all() and np.isfinite(sd).all()


def test_dense_rows_in_any_order(models):
    """A dense model whose rows are a permutation of the grid: y is reordered to grid order, z stays indexed by the grid."""
    gpim_amd, made, full, Xf = models
    r = made["dense"]
    z = np.random.default_rng(2).standard_normal((2, 3 * 256))
    want = r.sample(n_samples=2, z=z, method="blocks")
    X0, y0 = r._Xd, r._yd
    perm = torch.from_numpy(np.random.default_rng(3).permutation(256)).to(r._dev)
    try:
        r.model.X, r.model.y = X0[perm], y0[perm]
        assert np.array_equal(r.sample(n_samples=2, z=z, method="blocks"), want)
    finally:
        r.model.X, r.model.y = X0, y0


def test_refusals(models):
    gpim_amd, made, full, Xf = models
    r = made["reflection"]
    grid_before = (r.Xtest, r._Xtest_d, r.fulldims)
    before = r.sample(n_samples=1, seed=4, method="blocks")

    def unchanged(model=r, grid=grid_before, ref=before):
        assert model.Xtest is grid[0] and model._Xtest_d is grid[1] and model.fulldims == grid[2]
        assert np.array_equal(ref, model.sample(n_samples=1, seed=4, method="blocks"))

    with pytest.raises(ValueError, match="method must be"):
        r.sample(method="matheron")
    # jitter outside (0, s]
    for bad in (10.0, 0.0, -1e-6):
        with pytest.raises(ValueError, match="jitter"):
            r.sample(method="blocks", jitter=bad)
    # a wrong width of z: the joint route's and the pathwise route's for noisy draws with N = M
    for W in (256, 512):
        with pytest.raises(ValueError, match="shape"):
            r.sample(n_samples=1, z=np.zeros((1, W)), method="blocks")
    # an Xtest other than the training grid: moved by half a pixel, and a finer grid that holds every training row
    with pytest.raises(NotImplementedError, match="not on it"):
        r.sample(Xtest=Xf + 0.5, method="blocks")
    fine = np.array(np.meshgrid(np.arange(0.0, 15.5, 0.5), np.arange(0.0, 15.5, 0.5), indexing="ij"))
    with pytest.raises(NotImplementedError, match=r"grid point \(0, 1\) has none"):
        r.sample(Xtest=fine, method="blocks")
    Xnan = Xf.astype(np.float64)
    Xnan[:, 3, 4] = np.nan
    with pytest.raises(ValueError):
        r.sample(Xtest=Xnan, method="blocks")
    unchanged()
    # the Kronecker model keeps its test axes through a refused grid as well
    k = made["kronecker"]
    kb = k.sample(n_samples=1, seed=4, method="blocks")
    with pytest.raises(NotImplementedError):
        k.sample(Xtest=fine, method="blocks")
    assert np.array_equal(kb, k.sample(n_samples=1, seed=4, method="blocks"))
    mean, _ = k.predict(verbose=0)
    assert mean.shape == (16, 16)
    # a NaN image: the border solver, and the dense model with fewer observations than grid points
    R = full.copy()
    R[3, 4] = R[9, 2] = np.nan
    Xs = gpim_amd.utils.get_sparse_grid(R)
    kw = dict(kernel="Matern52", lengthscale=[[1., 1.], [8., 8.]], iterations=1, verbose=0)
    sk = gpim_amd.skreconstructor(Xs, R, Xf, **kw)
    assert sk.solver == "border"
    with pytest.raises(NotImplementedError, match="fully observed grid"):
        sk.sample(method="blocks")
    dn = gpim_amd.reconstructor(Xs, R, Xf, **kw)
    with pytest.raises(NotImplementedError, match=r"grid point \(3, 4\) has none"):
        dn.sample(method="blocks")
    for model in (sk, dn):
        mean, sd = model.predict(verbose=0)
        assert model.fulldims == (16, 16) and np.isfinite(mean).all()
    # sparse and single-precision models
    for model, why in ((gpim_amd.reconstructor(Xs, R, Xf, sparse=True, indpoints=20, iterations=1, verbose=0), "sparse=True"),
                       (gpim_amd.reconstructor(Xf, full, Xf, precision="single", iterations=1, verbose=0), "precision='single'"),
                       (gpim_amd.reconstructor(Xf, full, Xf, precision="single", structured=True, iterations=1, verbose=0),
                        "precision='single'")):
        with pytest.raises(NotImplementedError, match=why):
            model.sample(method="blocks")
        mean, _ = model.predict(verbose=0)
        assert np.isfinite(mean).all()
    # a grid without a symmetric axis
    ax = np.concatenate([np.arange(15.0), [20.0]])
    Xu = np.array(np.meshgrid(ax, ax, indexing="ij"))
    un = gpim_amd.reconstructor(Xu, full, Xu, kernel="Matern52", lengthscale=[[1., 1.], [8., 8.]], iterations=1, verbose=0)
    with pytest.raises(NotImplementedError, match="symmetric"):
        un.sample(method="blocks")
    assert np.isfinite(un.predict(verbose=0)[0]).all()
    # the other methods keep their refusal of structured models
    with pytest.raises(NotImplementedError, match="dense double-precision engine"):
        r.sample(method="pathwise")
    with pytest.raises(NotImplementedError, match="dense double-precision engine"):
        r.sample()
    unchanged()


def test_not_pd_leaves_the_model_usable(models):
    """RBF with a lengthscale 20 x the grid and jitter 1e-30: the prior blocks are numerically singular.  numpy's Cholesky
    fails on them too; the library reports it through the one status word and the reconstructor stays usable."""
    gpim_amd, made, full, Xf = models
    from gpim_amd import _lib
    r = gpim_amd.reconstructor(Xf, full, Xf, kernel="RBF", lengthscale=[[320., 320.], [321., 321.]], jitter=1e-30, iterations=1,
                               verbose=0)
    P, blocks = oracle_params(r), blocks_of((16, 16))
    with pytest.raises(np.linalg.LinAlgError):
        for Kb in blocks.prior_blocks(P, 1e-30):
            np.linalg.cholesky(Kb)
    with pytest.raises(_lib.NotPositiveDefiniteError):
        r.sample(method="blocks")
    ok = r.sample(n_samples=2, seed=0, method="blocks", jitter=0.5 * P.noise)
    assert ok.shape == (2, 16, 16) and np.isfinite(ok).all()
    mean, sd = r.predict(verbose=0)
    assert np.isfinite(mean).all() and np.isfinite(sd).all()
