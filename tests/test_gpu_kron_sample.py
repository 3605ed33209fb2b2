"""
Posterior draws of the Kronecker model on any product test grid on the MI355X:
reconstructor.sample(method='kron') / gpimhip_sample_kron against the dense numpy oracle of tests/kron_sample_oracle.py.

A draw is ``mean + A z``; the root of the prior fixes A only up to an orthogonal change of zeta, so the device is held to the
oracle through the covariance: one call with z = I returns A, and A A^T must be Sigma_post + c I of the Cholesky posterior.
Bar: 1e-9 max(1, s2), what tests/test_gpu_kron.py holds the Kronecker variance to (the same eigen-decompositions and mode
products produce both).  Hyper-parameters are fixed by writing u; lengthscale bounds [[0.1] * d, [10] * d].
"""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kron_sample_oracle as KO


@pytest.fixture(scope="module")
def gpim(ensure_built):
    import gpim_amd
    return gpim_amd


# beyond the host test's cases: union axes of order 39 and 23 (centro-symmetric: the split eigen-problems), S = 2034 draws in
# one call; 40x4-shifted: a union axis of order 80, centro-symmetric too (c_a + c_{79-a} = 39.37), so two problems of order
# 40; 40x4-skewed: shifts that grow along the axis break the symmetry -- one eigen-problem of order 80, the eigen-solver's
# instantiation above order 64
EXTRA = {
    "20x12-finer": ((np.arange(20.0), np.arange(12.0)), (np.arange(0, 19.5, .5), np.arange(0, 11.5, .5))),
    "40x4-shifted": ((np.arange(40.0), np.arange(4.0)), (np.arange(40.0) + 0.37, np.arange(4.0))),
    "40x4-skewed": ((np.arange(40.0), np.arange(4.0)), (np.arange(40.0) + 0.2 + 0.005 * np.arange(40.0), np.arange(4.0))),
}
ALL_CASES = KO.CASES + tuple((name, k) for name in EXTRA for k in (0, 1))


def case(name, k):
    if name in EXTRA:
        return EXTRA[name] + KO.PARAMS_2D[k]
    return KO.case(name, k)


def grid_of(axes):
    return np.array(np.meshgrid(*axes, indexing="ij"))


def observations(c):
    P = KO.points(c)
    y = np.sin(P.sum(1) / 3.0) + 0.1 * np.random.default_rng(len(P)).standard_normal(len(P))
    return y.reshape([len(a) for a in c])


def set_params(rec, ls, s2, noise):
    """writes u so that the constrained values are (s2, ls, noise) to rounding; returns the values the engine holds"""
    sp = rec._spec
    p = torch.cat([torch.tensor([(s2 - sp.amp_lo) / (sp.amp_hi - sp.amp_lo)], dtype=torch.float64),
                   (torch.tensor(ls, dtype=torch.float64) - sp.ls_lo) / (sp.ls_hi - sp.ls_lo)])
    u = torch.cat([torch.logit(p), torch.tensor([math.log(noise)], dtype=torch.float64)])
    rec._u[:u.numel()].copy_(u.to(rec._u.device))          # (a sparse model keeps its inducing inputs behind them)
    var, lsc, nz = sp.constrained(rec._u)
    return lsc.tolist(), float(var), float(nz)


def build(gpim, c, ls, s2, noise, Xtest=None, cls=None, **kw):
    d = len(c)
    R = observations(c)
    cls = cls or gpim.reconstructor
    kw.setdefault("structured", True)
    rec = cls(grid_of(c), R, Xtest, kernel=kw.pop("kernel", "RBF"), lengthscale=[[0.1] * d, [10.0] * d], verbose=0, **kw)
    return rec, R, set_params(rec, ls, s2, noise)


def draw_matrix_device(rec, t, noiseless, jitter, **kw):
    """A of the device, (M, W), from one call with z = I, and the predicted mean (M,)"""
    PU, N, M = KO.widths(rec._solver.axes, t)
    W = PU + N + M
    Xt = grid_of(t)
    out = rec.sample(n_samples=W, Xtest=Xt, z=np.eye(W), noiseless=noiseless, jitter=jitter, method="kron", **kw)
    assert out.shape == (W,) + Xt.shape[1:]
    mean = rec.predict(Xt)[0].reshape(-1)
    return (out.reshape(W, M) - mean).T, mean


@pytest.mark.parametrize("name,k", ALL_CASES, ids=lambda v: str(v))
def test_distribution_is_the_posterior(gpim, name, k):
    c, t, ls, s2, noise = case(name, k)
    rec, R, (ls_e, s2_e, noise_e) = build(gpim, c, ls, s2, noise)
    mean_o, cov = KO.posterior(c, t, ls_e, s2_e, noise_e, KO.MODEL_JITTER, R)
    M = cov.shape[0]
    bar = 1e-9 * max(1.0, s2)
    for noiseless in (False, True):
        A, mean = draw_matrix_device(rec, t, noiseless, KO.MODEL_JITTER)
        cc = (0.0 if noiseless else noise_e) + KO.MODEL_JITTER
        err = np.abs(A @ A.T - (cov + cc * np.eye(M))).max()
        print("%s/%d noiseless=%d W=%d: max|A A^T - (Sigma_post + c I)| = %.3e (bar %.1e), mean - oracle %.3e"
              % (name, k, noiseless, A.shape[1], err, bar, np.abs(mean - mean_o).max()))
        assert np.isfinite(A).all()
        assert err <= bar
        assert np.abs(mean - mean_o).max() <= 1e-9


@pytest.mark.parametrize("name", ("finer", "crop", "3d"))
def test_mean_and_structure(gpim, name):
    c, t, ls, s2, noise = case(name, 0)
    rec, R, _ = build(gpim, c, ls, s2, noise)
    Xt = grid_of(t)
    PU, N, M = KO.widths(c, t)
    W = PU + N + M
    mean0, sd0 = rec.predict(Xt)
    # z = 0: the mean of predict()
    out = rec.sample(n_samples=2, z=np.zeros((2, W)), method="kron")
    assert out.shape == (2,) + Xt.shape[1:]
    assert np.abs(out - mean0).max() <= 1e-9
    # S = 3 random rows: mean + A z, row by row (no draw leaks into another)
    A, mean = draw_matrix_device(rec, t, False, KO.MODEL_JITTER)
    Z = np.random.default_rng(5).standard_normal((3, W))
    out = rec.sample(n_samples=3, z=Z, method="kron").reshape(3, M)
    ref = mean + Z @ A.T
    err = np.abs(out - ref).max()
    print("%s: S=3 draws - (mean + A z) = %.3e (bar %.3e)" % (name, err, 1e-11 * np.abs(out).max()))
    assert err <= 1e-11 * np.abs(out).max()
    # seeded draws repeat; z as an array and as a device tensor are the same call
    a, b = rec.sample(3, seed=11, method="kron"), rec.sample(3, seed=11, method="kron")
    assert np.array_equal(a, b) and not np.array_equal(a, rec.sample(3, seed=12, method="kron"))
    assert np.array_equal(rec.sample(3, z=torch.from_numpy(Z).cuda(), method="kron").reshape(3, M), out)
    # noiseless with jitter 0: nothing of z_n reaches the draw
    A0, _ = draw_matrix_device(rec, t, True, 0.0)
    assert not A0[:, PU + N:].any() and A0[:, :PU + N].any()
    # predict() is what it was
    mean1, sd1 = rec.predict(Xt)
    assert np.array_equal(mean1, mean0) and np.array_equal(sd1, sd0)


def test_against_the_joint_draws_of_the_dense_model(gpim):
    """On the training grid (16 x 16) the covariance of method='kron' is that of the dense model's method='joint' at the
    same jitter, each recovered from one call with z = I."""
    c = (np.arange(16.0), np.arange(16.0))
    ls, s2, noise, j = [2.0, 3.0], 1.7, 0.02, 3e-4
    rec, R, _ = build(gpim, c, ls, s2, noise)
    den, _, _ = build(gpim, c, ls, s2, noise, structured=False)
    assert type(den._solver).__name__ == "Dense" and torch.equal(den._u, rec._u)
    M = 256
    for noiseless in (False, True):
        A, mean = draw_matrix_device(rec, c, noiseless, j)
        out = den.sample(n_samples=M, Xtest=grid_of(c), z=np.eye(M), noiseless=noiseless, jitter=j, method="joint")
        B = (out.reshape(M, M) - den.predict(grid_of(c))[0].reshape(-1)).T
        err = np.abs(A @ A.T - B @ B.T).max()
        print("16x16 noiseless=%d: max|A A^T (kron) - A A^T (joint)| = %.3e (bar %.1e)" % (noiseless, err, 1e-9 * max(1, s2)))
        assert err <= 1e-9 * max(1.0, s2)


def test_refused_models(gpim):
    from gpim_amd import _solvers
    c = (np.arange(8.0), np.arange(8.0))
    models = (dict(structured=False), dict(kernel="Matern52"), dict(structured=False, sparse=True),
              dict(structured=False, precision="single"), dict(precision="single"))
    for kw in models:
        rec, _, _ = build(gpim, c, [2.0, 2.0], 1.0, 0.05, **dict(kw))
        with pytest.raises(NotImplementedError, match="method='kron'"):
            rec.sample(2, seed=0, method="kron")
        if not isinstance(rec._solver, _solvers.Kron):
            with pytest.raises(NotImplementedError, match="Kronecker"):
                rec._solver.sample_kron(rec)


def test_entry_point_limits(gpim):
    """gpimhip_sample_kron refuses a union axis beyond the eigen-solver's 4096 (naming the axis), S < 1 and a negative
    jitter before it allocates or launches anything.  Every buffer has the size its arguments declare."""
    from gpim_amd import _lib
    i32 = lambda v: (ctypes.c_int32 * len(v))(*[int(k) for k in v])
    buf = lambda k: torch.zeros(int(k), dtype=torch.float64, device="cuda")

    def call(rec, c, t, S, jitter):
        au, ic, it = gpim.utils.union_axes(c, t)
        PU, N, M = KO.widths(c, t)
        args = [buf(sum(len(a) for a in c)), buf(N), buf(sum(len(a) for a in t)), buf(sum(len(a) for a in au)),
                buf(max(S, 1) * (PU + N + M)), buf(M), buf(max(S, 1) * M)]
        ax, y, tx, ux, z, mean, out = (_lib.ptr(a) for a in args)
        lib, h = rec._handle.lib, rec._handle.h
        bytes0 = lib.gpimhip_workspace_bytes(h)
        rc = lib.gpimhip_sample_kron(h, ctypes.byref(rec._mstruct), len(c), i32([len(a) for a in c]), ax, y, _lib.ptr(rec._u),
                                     i32([len(a) for a in t]), tx, i32([len(a) for a in au]), ux, i32(np.concatenate(ic)),
                                     i32(np.concatenate(it)), z, S, 0, jitter, mean, out)
        assert lib.gpimhip_workspace_bytes(h) == bytes0
        return rc, lib.gpimhip_last_error().decode()

    small = (np.arange(4.0), np.arange(4.0))
    rec, _, _ = build(gpim, small, [2.0, 2.0], 1.0, 0.05)
    c, t = (np.arange(2.0), np.arange(4000.0)), (np.arange(2.0), np.arange(200.0) + 0.5)
    rc, msg = call(rec, c, t, 1, 1e-5)
    assert rc == _lib.E_BADARG and "axis 1" in msg and "4200" in msg and "4096" in msg
    rc, msg = call(rec, small, small, 0, 1e-5)
    assert rc == _lib.E_BADARG and "S >= 1" in msg
    rc, msg = call(rec, small, small, 1, -1e-6)
    assert rc == _lib.E_BADARG and "jitter" in msg
    big, _, _ = build(gpim, c, [2.0, 2.0], 1.0, 0.05)
    with pytest.raises(NotImplementedError, match="axis 1.*4200.*4096"):
        big.sample(1, seed=0, Xtest=grid_of(t), method="kron")


def test_refused_arguments_leave_the_model_alone(gpim):
    c, t, ls, s2, noise = case("shifted", 0)          # (PU = 84, N = 30, M = 42: no wrong width below happens to be right)
    rec, R, _ = build(gpim, c, ls, s2, noise, Xtest=grid_of(t))
    PU, N, M = KO.widths(c, t)
    W = PU + N + M
    before = rec.sample(2, seed=3, method="kron")
    kept = (rec.Xtest, rec._Xtest_d, rec.fulldims, rec._solver.taxes)
    Xnan = grid_of(c)
    Xnan[0, 1, 2] = np.nan
    Xbad = grid_of(c)
    Xbad[0, 3, 4] += 0.5
    refusals = [
        (ValueError, "finite", dict(Xtest=Xnan)),
        (NotImplementedError, "product grid", dict(Xtest=Xbad)),
        (ValueError, "jitter", dict(jitter=-1e-6)),
        (ValueError, "zeta", dict(z=np.zeros((2, M)))),
        (ValueError, "zeta", dict(z=np.zeros((2, 2 * M + N)))),
        (ValueError, "zeta", dict(z=np.zeros((2, PU + N)))),
        (ValueError, "zeta", dict(z=np.zeros((3, W)))),
        (ValueError, "method must be.*'border'.*'kron'", dict(method="matheron")),
    ]
    for exc, match, kw in refusals:
        kw.setdefault("method", "kron")
        with pytest.raises(exc, match=match):
            rec.sample(2, seed=3, **kw)
        now = (rec.Xtest, rec._Xtest_d, rec.fulldims, rec._solver.taxes)
        assert all(a is b for a, b in zip(kept, now)), kw
        assert np.array_equal(rec.sample(2, seed=3, method="kron"), before), kw
    # an accepted call with a new grid stores it, as predict() does
    out = rec.sample(2, seed=3, Xtest=grid_of(c), method="kron")
    assert out.shape == (2, 6, 5) and tuple(rec.fulldims) == (6, 5) and rec._solver.taxes is not kept[3]


def test_through_skreconstructor(gpim):
    R = observations((np.arange(8.0), np.arange(8.0)))
    X_full = gpim.utils.get_full_grid(R)
    fine = gpim.utils.get_full_grid(R, dense_x=0.5)
    rec = gpim.skreconstructor(X_full, R, X_full, "RBF", verbose=0)
    assert rec.solver == "kronecker"
    out = rec.sample(4, seed=0, Xtest=fine, method="kron", noiseless=True)
    assert out.shape == (4,) + fine.shape[1:] and np.isfinite(out).all()
    mean, sd = rec.predict(fine)
    noise = float(rec._spec.constrained(rec._u)[2])
    sd_f = np.sqrt(np.maximum(sd ** 2 - noise, 0.0))
    dev = np.abs(out - mean)[:, ::2, ::2] / sd_f[::2, ::2]
    print("skreconstructor 8x8 -> 16x16: largest |draw - mean| / sd at the training pixels = %.2f" % dev.max())
    assert dev.max() <= 6.0
