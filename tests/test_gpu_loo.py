"""
Leave-one-out cross-validation on the MI355X (gpimhip_loo_exact / _exact_batched / _kron, reconstructor.loo) against the
float64 references of tests/loo_oracle.py: `brute` (N refits of the dense oracle) where N allows, `closed` (the identity in
numpy, held to `brute` by tests/test_loo_host.py) beyond.  The bars are the project's own for the same quantities:
  dense, double      mean and variance atol 1e-10   (test_gpu_ops.test_kmat_nll_grad_predict's posterior bar)
  dense, single      against the double engine: mean atol 2e-3 (max|mean| + 1), variance rtol 2e-2 / atol 1e-4 (test_gpu_single.py)
  reflection, Kron   atol 1e-9                      (the small-size structured posterior bar of test_gpu_kron.py)
  score              rtol 1e-12 against a float64 recomputation from the returned arrays
Every test prints the distances it measured before it asserts.
"""
import ctypes

import numpy as np
import pytest
import torch
from numpy.testing import assert_allclose

pytestmark = pytest.mark.gpu

import loo_oracle as LO


@pytest.fixture(scope="module")
def eng(ensure_built):
    from gpim_amd import _lib
    H = _lib.Handle()
    yield _lib, H
    H.close()


def loo_abi(_lib, H, spec, u, X, y):
    """(mean, var, score) numpy arrays of gpimhip_loo_exact on the handle H"""
    N = X.shape[0]
    m = spec.struct()
    Xd, yd, ud = X.cuda().contiguous(), y.cuda().contiguous(), u.cuda()
    mean = torch.full((N + 3,), -7.0, dtype=torch.float64, device="cuda")      # three sentinels: only N entries are written
    var = torch.full((N + 3,), -7.0, dtype=torch.float64, device="cuda")
    score = torch.empty(2, dtype=torch.float64, device="cuda")
    _lib.check(H.lib.gpimhip_loo_exact(H.h, ctypes.byref(m), _lib.ptr(Xd), _lib.ptr(yd), N, _lib.ptr(ud), _lib.ptr(mean),
                                       _lib.ptr(var), _lib.ptr(score)))
    mh, vh = mean.cpu().numpy(), var.cpu().numpy()
    assert np.all(mh[N:] == -7.0) and np.all(vh[N:] == -7.0)
    return mh[:N], vh[:N], score.cpu().numpy()


# N = 40: one padded block; 130: the second block holds 2 rows; 300: isotropic; 530: np = 640, five row chunks, the last
# block ragged with 18 valid rows (its padding rows are never written by the factorisation, and never read here)
DENSE = [(40, 2, False), (130, 3, False), (300, 2, True), (530, 3, False)]


@pytest.mark.parametrize("kind", ["RBF", "Matern52", "RationalQuadratic"])
@pytest.mark.parametrize("N,d,iso", DENSE)
def test_dense_loo(eng, kind, N, d, iso):
    _lib, H = eng
    kp, spec, u, X, y = LO.problem(kind, N, d, iso)
    assert len(X) == N
    mref, vref = LO.dense_reference(kind, N, d, iso)
    mean, var, score = loo_abi(_lib, H, spec, u, X, y)
    print("%s N=%d: max |mean - ref| %.2e, max |var - ref| %.2e" % (kind, N, np.abs(mean - mref).max(), np.abs(var - vref).max()))
    assert_allclose(mean, mref, rtol=0, atol=1e-10)
    assert_allclose(var, vref, rtol=0, atol=1e-10)
    elpd, sse = LO.score(mean, var, y.numpy())
    assert_allclose(score, [elpd, sse], rtol=1e-12)


def test_dense_loo_4212(eng):
    """N = 4212, d = 3, Matern52: the first matrix order with 256-row chunks (np = 4224: 16 full chunks and one of 128 rows).
    Reference: `closed` (two float64 evaluations of it differ by 2e-14 here; condition number 1.3e3)."""
    _lib, H = eng
    kp, spec, u, X, y = LO.problem("Matern52", 4212, 3, False)
    assert len(X) == 4212
    mref, vref = LO.closed(kp, X, y)
    mean, var, score = loo_abi(_lib, H, spec, u, X, y)
    print("Matern52 N=4212: max |mean - ref| %.2e, max |var - ref| %.2e" % (np.abs(mean - mref).max(), np.abs(var - vref).max()))
    assert_allclose(mean, mref, rtol=0, atol=1e-10)
    assert_allclose(var, vref, rtol=0, atol=1e-10)
    assert_allclose(score, LO.score(mean, var, y.numpy()), rtol=1e-12)


def test_score_and_reproducibility(eng):
    _lib, H = eng
    kp, spec, u, X, y = LO.problem("Matern52", 530, 3, False)
    a = loo_abi(_lib, H, spec, u, X, y)
    elpd, sse = LO.score(a[0], a[1], y.numpy())
    print("N=530: elpd %.12g (host %.12g), sse %.12g (host %.12g)" % (a[2][0], elpd, a[2][1], sse))
    assert_allclose(a[2], [elpd, sse], rtol=1e-12)
    b = loo_abi(_lib, H, spec, u, X, y)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    # a handle that has fitted another problem of the same padded order, one that fills the last block (N = 600: every row
    # of the workspace matrices written), gives the bits of a fresh handle
    from gpim_amd.kernels import KernelSpec
    used = _lib.Handle()
    try:
        X6, y6 = LO.scattered(600, 2, seed=600, grid=64)
        s6 = KernelSpec("RBF", 2, [[1., 1.], [20., 20.]], jitter=1e-5)
        u6 = s6.draw_initial_u(generator=torch.Generator().manual_seed(6)).cuda()
        m6 = s6.struct()
        X6d, y6d = X6.cuda().contiguous(), y6.cuda().contiguous()
        _lib.check(used.lib.gpimhip_fit_exact(used.h, ctypes.byref(m6), _lib.ptr(X6d), _lib.ptr(y6d), len(X6), _lib.ptr(u6), 0.1,
                                              3, None, None))
        c = loo_abi(_lib, used, spec, u, X, y)
    finally:
        used.close()
    assert all(np.array_equal(p, q) for p, q in zip(a, c))


@pytest.mark.parametrize("N,d,iso", [(300, 2, True), (530, 3, False)])
def test_single_precision_loo(eng, N, d, iso):
    """The single-precision engine against the double engine on the same model.  (A float32 factor on the CPU gave mean
    <= 3.6e-7 and variance relative error <= 9.5e-7: an estimate for another factorisation, not the bar.)"""
    _lib, H = eng
    kp, spec, u, X, y = LO.problem("Matern52", N, d, iso)
    m64, v64, s64 = loo_abi(_lib, H, spec, u, X, y)
    H32 = _lib.Handle(precision="single")
    try:
        m32, v32, s32 = loo_abi(_lib, H32, spec, u, X, y)
    finally:
        H32.close()
    print("single N=%d: max |mean - double| %.2e, max rel |var - double| %.2e, elpd %.6f vs %.6f"
          % (N, np.abs(m32 - m64).max(), (np.abs(v32 - v64) / v64).max(), s32[0], s64[0]))
    assert_allclose(m32, m64, rtol=0, atol=2e-3 * (np.abs(m64).max() + 1))
    assert_allclose(v32, v64, rtol=2e-2, atol=1e-4)
    assert_allclose(s32, LO.score(m32, v32, y.numpy()), rtol=1e-12)


def grid_model(gpim, cls, shape, kind, ls, noise_u, **kw):
    """A reconstructor on the complete grid of `shape` at its initial parameters with u_noise = noise_u, and the oracle's
    parameters at the same u"""
    d = len(shape)
    R = LO.smooth_grid(shape, seed=sum(shape))
    Xg = gpim.utils.get_full_grid(R)
    rec = cls(Xg, R, kernel=kind, lengthscale=ls, iterations=0, verbose=0, **kw)
    rec._u[1 + rec._spec.n_ls] = noise_u
    return rec, R, LO.kp_from_u(kind, d, ls, rec._u)


@pytest.mark.parametrize("kind", ["Matern52", "RationalQuadratic"])
@pytest.mark.parametrize("shape", [(6, 5), (5, 5), (4, 3, 4), (16, 12)])
def test_reflection_loo(ensure_built, kind, shape):
    """reconstructor(structured=True) through the reflection blocks (B = 4 or 8; mirror planes on the axes of odd length)
    against N refits of the dense oracle at the same u, and against the dense reconstructor's own loo()"""
    import gpim_amd
    d = len(shape)
    ls = [[0.5] * d, [12.0] * d]
    rec, R, kp = grid_model(gpim_amd, gpim_amd.reconstructor, shape, kind, ls, -3.0, structured=True)
    assert rec.do_symm and rec._solver.S["B"] == 2 ** d
    mean, sd, score = rec.loo()
    assert mean.shape == R.shape and sd.shape == R.shape and score["n"] == R.size
    mref, vref = LO.brute(kp, rec.X, rec.y)
    print("%s %s: max |mean - ref| %.2e, max |var - ref| %.2e" % (kind, shape, np.abs(mean.ravel() - mref).max(),
                                                                 np.abs(sd.ravel() ** 2 - vref).max()))
    assert_allclose(mean.ravel(), mref, rtol=0, atol=1e-9)
    assert_allclose(sd.ravel() ** 2, vref, rtol=0, atol=1e-9)
    dense = gpim_amd.reconstructor(gpim_amd.utils.get_full_grid(R), R, kernel=kind, lengthscale=ls, iterations=0, verbose=0)
    dense._u.copy_(rec._u)
    md, sdd, scd = dense.loo()
    assert_allclose(mean, md, rtol=0, atol=1e-9)
    assert_allclose(sd ** 2, sdd ** 2, rtol=0, atol=1e-9)
    elpd, sse = LO.score(mean, sd ** 2, R)
    assert_allclose([score["elpd"], score["rmse"]], [elpd, np.sqrt(sse / R.size)], rtol=1e-11)
    assert_allclose(score["elpd"], scd["elpd"], rtol=0, atol=1e-7 * R.size)


@pytest.mark.parametrize("shape", [(9, 8), (6, 5, 4)])
def test_kron_loo(ensure_built, shape):
    """skreconstructor(kernel='RBF') on a complete grid (the Kronecker solver) at the noise level of test_gpu_kron.py's small
    cases, against N refits of the dense oracle at the same u"""
    import gpim_amd
    d = len(shape)
    ls = [[0.7] * d, [9.0] * d]
    rec, R, kp = grid_model(gpim_amd, gpim_amd.skreconstructor, shape, "RBF", ls, -2.5)
    assert rec.solver == "kronecker"
    mean, sd, score = rec.loo()
    mref, vref = LO.brute(kp, rec.X, rec.y)
    print("RBF %s: max |mean - ref| %.2e, max |var - ref| %.2e" % (shape, np.abs(mean.ravel() - mref).max(),
                                                                  np.abs(sd.ravel() ** 2 - vref).max()))
    assert mean.shape == R.shape
    assert_allclose(mean.ravel(), mref, rtol=0, atol=1e-9)
    assert_allclose(sd.ravel() ** 2, vref, rtol=0, atol=1e-9)
    elpd, sse = LO.score(mean, sd ** 2, R)
    assert_allclose([score["elpd"], score["rmse"]], [elpd, np.sqrt(sse / R.size)], rtol=1e-11)


def sparse_image(shape=(14, 12), keep=0.6, seed=4):
    R = LO.smooth_grid(shape, seed)
    R[np.random.default_rng(seed).uniform(size=shape) > keep] = np.nan
    return R


@pytest.mark.parametrize("precision", ["double", "single"])
def test_python_surface(eng, precision):
    import gpim_amd
    _lib, H = eng
    R = sparse_image()
    X = gpim_amd.utils.get_sparse_grid(R)
    rec = gpim_amd.reconstructor(X, R, kernel="RBF", lengthscale=[[0.5, 0.5], [12., 12.]], iterations=0, verbose=0,
                                 precision=precision)
    rec._u[1 + rec._spec.n_ls] = -3.0
    mean, sd, score = rec.loo()
    obs = ~np.isnan(R)
    N = int(obs.sum())
    dt = np.float32 if precision == "single" else np.float64
    assert mean.shape == R.shape and sd.shape == R.shape and mean.dtype == dt and sd.dtype == dt
    assert np.array_equal(np.isnan(mean), ~obs) and np.array_equal(np.isnan(sd), ~obs)
    mf, sf, score_f = rec.loo(as_grid=False)
    assert mf.shape == (N,) and np.array_equal(mf, mean[obs]) and np.array_equal(sf, sd[obs]) and score_f == score
    assert score["n"] == N and set(score) == {"elpd", "rmse", "n"}
    # the C entry on a handle of the same precision, at the model's parameters
    Hp = H if precision == "double" else _lib.Handle(precision="single")
    try:
        ma, va, sa = loo_abi(_lib, Hp, rec._spec, rec._u.cpu(), rec._Xd.cpu(), rec._yd.cpu())
    finally:
        if Hp is not H:
            Hp.close()
    assert np.array_equal(mf, ma.astype(dt)) and np.array_equal(sf, np.sqrt(va).astype(dt))
    assert score["elpd"] == sa[0] and score["rmse"] == np.sqrt(sa[1] / N)
    # new training data through model.X / model.y no longer belong to the constructor's grid
    keep = np.arange(N) % 3 != 0
    rec.model.X = rec._Xd[torch.from_numpy(keep).cuda()]
    rec.model.y = rec._yd[torch.from_numpy(keep).cuda()]
    with pytest.raises(ValueError, match="as_grid=False"):
        rec.loo()
    assert rec.loo(as_grid=False)[0].shape == (int(keep.sum()),)


def matern_prior_image(shape=(18, 16), ls=3.0, noise=0.01, seed=1):
    idx = np.array(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")).reshape(2, -1).T
    r = np.sqrt(((idx[:, None, :] - idx[None, :, :]) ** 2).sum(-1)) / ls
    K = (1 + np.sqrt(5) * r + 5. / 3 * r * r) * np.exp(-np.sqrt(5) * r)
    rng = np.random.default_rng(seed)
    f = np.linalg.cholesky(K + 1e-10 * np.eye(len(K))) @ rng.standard_normal(len(K))
    return (f + np.sqrt(noise) * rng.standard_normal(len(K))).reshape(shape)


def test_elpd_prefers_the_kernel_that_generated_the_data(ensure_built):
    """README's example: an image drawn from a Matern52 prior (lengthscale 3, noise 0.01), a Matern52 and an RBF model
    trained alike (50 iterations, seed 0).  The CPU oracle's trajectories give elpd 142.7 and 91.7."""
    import gpim_amd
    R = matern_prior_image()
    X = gpim_amd.utils.get_full_grid(R)
    elpd = {}
    for kern in ("Matern52", "RBF"):
        rec = gpim_amd.reconstructor(X, R, kernel=kern, lengthscale=[[1., 1.], [10., 10.]], learning_rate=0.1, iterations=50,
                                     verbose=0, seed=0)
        rec.train()
        elpd[kern] = rec.loo()[2]["elpd"]
    print("elpd: Matern52 %.3f, RBF %.3f" % (elpd["Matern52"], elpd["RBF"]))
    assert elpd["Matern52"] > elpd["RBF"]


def test_refusals(ensure_built):
    import gpim_amd
    from gpim_amd import _lib, _solvers, gprutils
    kw = dict(iterations=0, verbose=0)
    R = sparse_image()
    with pytest.raises(NotImplementedError, match="Sparse.*inducing"):
        gpim_amd.reconstructor(gpim_amd.utils.get_sparse_grid(R), R, sparse=True, indpoints=20, **kw).loo()
    # three missing pixels: the bordered reflection blocks
    Rb = LO.smooth_grid((24, 20), 3)
    Rb[3, 4] = Rb[10, 11] = Rb[20, 2] = np.nan
    rb = gpim_amd.skreconstructor(gpim_amd.utils.get_sparse_grid(Rb), Rb, kernel="Matern52", **kw)
    assert rb.solver == "border"
    with pytest.raises(NotImplementedError, match="Reflection.*border"):
        rb.loo()
    # two whole rows missing: the dense-by-Kronecker blocks
    Rc = LO.smooth_grid((12, 10), 3)
    Rc[[2, 7], :] = np.nan
    rc = gpim_amd.skreconstructor(gpim_amd.utils.get_sparse_grid(Rc), Rc, kernel="RBF", **kw)
    assert rc.solver == "columns"
    with pytest.raises(NotImplementedError, match="Columns.*columns"):
        rc.loo()
    # structured solvers on a single-precision model
    Rf = LO.smooth_grid((8, 6), 2)
    Xf = gpim_amd.utils.get_full_grid(Rf)
    for kern, name in (("RBF", "Kron"), ("Matern52", "Reflection")):
        with pytest.raises(NotImplementedError, match=name + ".*precision='double'"):
            gpim_amd.reconstructor(Xf, Rf, kernel=kern, structured=True, precision="single", **kw).loo()
    # the batched entry itself with a border set
    D = rb._solver
    with D._mode(rb) as blocks:
        n = blocks.n_total
        z = torch.zeros(n, dtype=torch.float64, device="cuda")
        zi = torch.zeros(n, dtype=torch.int32, device="cuda")
        u_b = rb._u.repeat(blocks.B).contiguous()
        rcode = rb._handle.lib.gpimhip_loo_exact_batched(*_solvers._head(rb), _lib.ptr(blocks.Xq), 0, _lib.ptr(blocks.ys),
                                                         blocks.Xq.shape[0], blocks.B, _lib.ptr(u_b),
                                                         ctypes.c_void_p(zi.data_ptr()), ctypes.c_void_p(zi.data_ptr()),
                                                         _lib.ptr(z), _lib.ptr(z), _lib.ptr(z), _lib.ptr(z))
    assert rcode == _lib.E_BADARG and b"border" in rb._handle.lib.gpimhip_last_error()
