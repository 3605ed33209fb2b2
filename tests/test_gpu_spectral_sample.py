"""
Posterior draws of the spectral-mixture GP on the MI355X: gpimhip_sample_sm, gpimhip_sample_sm_pathwise,
gpimhip_sample_sm_blocks and skreconstructor(kernel='Spectral').sample against the host oracle of tests/sm_sample_oracle.py on
the same standard normals -- device and oracle are both pure functions of z.

Bar of the draws: 10 x the host discrepancy recorded by tests/test_sm_sample_host.py (sm_sample_oracle.HOST_DISCREPANCY_OVER_SW,
the rounding level of the recipe in float64 relative to sum w) x sum w x the condition number reported for the case: the
largest among K + s I and the prior blocks K_b + d I (the joint matrix for 'joint'; the blocks K_b + d I and K_b + s I for
'blocks') -- the draws are forward quantities of their Cholesky factors.  The margin of 10 is for the different summation
order and the blocked factors, as in tests/test_gpu_pathwise.py.  Every case must have cond < 1e7 (asserted), so that the bar
stays far below a draw's magnitude.  The mean is held to gpimhip_predict_sm's and to the oracle's at the project's 1e-10
(ATOL_MEAN); the variance of 'joint' to sm_oracle.predict's at 1e-10 sum w.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
from numpy.testing import assert_allclose

pytestmark = pytest.mark.gpu

import pathwise_oracle as PO
import sm_oracle as SO
import sm_sample_oracle as SSO

ATOL_MEAN = 1e-10
COND_CAP = 1e7
JITTER = SSO.JITTER


@pytest.fixture(scope="module")
def eng(ensure_built):
    from gpim_amd import _lib
    H = _lib.Handle()
    yield _lib, H
    H.close()


def dev(t):
    return (torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t).cuda().contiguous()


def sm_struct(_lib, d, Q, D):
    sm = _lib.SmStruct()
    sm.dim, sm.mixtures, sm.ard = d, Q, 0 if D == 1 and d > 1 else 1
    return sm


def draw_bar(P, cond):
    assert cond < COND_CAP, "the case's condition number %.3e is not below %.0e" % (cond, COND_CAP)
    return 10.0 * SSO.HOST_DISCREPANCY_OVER_SW * P.var * cond


@functools.lru_cache(maxsize=None)
def blocks_of(shape):
    return SSO.Blocks(PO.full_grid(shape)[0])


def params(gen, Q, D, seed):
    return SSO.Params(SSO.GENERATORS[gen](Q, D, seed + 11 * Q), Q, D)


def grid_args(blocks, shape):
    return ((ctypes.c_int32 * len(shape))(*shape), sum(1 << k for k in blocks.dims), (ctypes.c_double * 4)(*list(blocks.S["twoc"])))


def predict_sm(_lib, H, P, X, y, Xs):
    d = X.shape[1]
    sm = sm_struct(_lib, d, P.Q, P.D)
    Xd, yd, ud, Sd = dev(X), dev(y), dev(P.u), dev(Xs)
    pm = torch.empty(len(Xs), dtype=torch.float64, device="cuda")
    pv = torch.empty_like(pm)
    _lib.check(H.lib.gpimhip_predict_sm(H.h, ctypes.byref(sm), _lib.ptr(Xd), _lib.ptr(yd), len(X), _lib.ptr(ud), _lib.ptr(Sd),
                                        len(Xs), _lib.ptr(pm), _lib.ptr(pv)))
    return pm.cpu().numpy(), pv.cpu().numpy()


# ---------------------------------------------------------------------------------------------- pathwise through the C ABI
def pathwise_call(_lib, H, P, blocks, shape, idx, y, Z, noiseless, jitter=JITTER, want_mean=True):
    """gpimhip_sample_sm_pathwise -> (samples (S, M), mean or None) on the host"""
    sm = sm_struct(_lib, len(shape), P.Q, P.D)
    S, M, N = Z.shape[0], blocks.M, len(idx)
    Gd, idxd, yd, ud, Zd = dev(blocks.G), dev(idx), dev(y), dev(P.u), dev(Z)
    out = torch.full((S, M), float("nan"), dtype=torch.float64, device="cuda")
    mean = torch.full((M,), float("nan"), dtype=torch.float64, device="cuda") if want_mean else None
    _lib.check(H.lib.gpimhip_sample_sm_pathwise(H.h, ctypes.byref(sm), _lib.ptr(Gd), *grid_args(blocks, shape),
                                                ctypes.c_void_p(idxd.data_ptr()), _lib.ptr(yd), N, _lib.ptr(ud), _lib.ptr(Zd), S,
                                                int(noiseless), float(jitter), _lib.ptr(mean), _lib.ptr(out)))
    return out.cpu().numpy(), (mean.cpu().numpy() if want_mean else None)


# N = 130 crosses a 128-row staging tile; 24x24 has a 144-point fundamental domain (crosses a 128-block) and M = 576 ends in a
# partial 256-lane workgroup; Q = 16 is the maximum (four or eight mixture chunks); a 5- and a 13-point axis have mirror-plane weights
PW_GRIDS = (((6, 5), 7, 3, False), ((6, 5), 30, 3, False), ((13, 10), 40, 16, True), ((24, 24), 130, 4, False),
            ((4, 3, 4), 9, 2, True))
PW_CASES = tuple(g + (gen, seed) for g in PW_GRIDS for gen in ("random_u", "narrow_u") for seed in (1, 2))


def pw_id(c):
    return "%s-N%d-Q%d-%s-%s-seed%d" % ("x".join(str(n) for n in c[0]), c[1], c[2], "iso" if c[3] else "ard", c[4], c[5])


@functools.lru_cache(maxsize=None)
def pw_problem(shape, N, Q, iso, gen, seed):
    d = len(shape)
    P = params(gen, Q, 1 if iso else d, seed)
    blocks = blocks_of(shape)
    idx = np.random.default_rng(N).permutation(blocks.M)[:N].astype(np.int64)
    X = blocks.G[idx]
    y = np.sin(X.sum(1) / 5.0) + 0.1 * np.random.default_rng(N + 1).standard_normal(N)
    return P, blocks, idx, y, SSO.condition(P, blocks, idx)


@pytest.mark.parametrize("case", PW_CASES, ids=pw_id)
def test_pathwise_against_oracle(eng, case):
    _lib, H = eng
    shape = case[0]
    P, blocks, idx, y, cond = pw_problem(*case)
    M, N = blocks.M, len(idx)
    tol = draw_bar(P, cond)
    pm, _ = predict_sm(_lib, H, P, blocks.G[idx], y, blocks.G)
    worst = 0.0
    for noiseless in (1, 0):
        W = M + N + (0 if noiseless else M)
        Z9 = np.random.default_rng(100 + noiseless).standard_normal((9, W))
        ref9 = SSO.draws(P, blocks, idx, y, Z9, noiseless)
        kept = {}
        for S in (9, 3, 1):                                  # 9 spans two groups (8 + 1)
            rows = slice(4, 5) if S == 1 else slice(0, S)
            out, mean = pathwise_call(_lib, H, P, blocks, shape, idx, y, Z9[rows], noiseless)
            err = np.abs(out - ref9["out"][rows]).max()
            worst = max(worst, err)
            print("%s noiseless=%d S=%d: draws - oracle %.3e (bar %.3e, cond %.3e, sum w %.3g), mean - predict %.3e, "
                  "mean - oracle %.3e" % (pw_id(case), noiseless, S, err, tol, cond, P.var, np.abs(mean - pm).max(),
                                          np.abs(mean - ref9["mean"]).max()))
            assert np.isfinite(out).all()
            assert_allclose(out, ref9["out"][rows], rtol=0, atol=tol)
            assert_allclose(mean, pm, rtol=0, atol=ATOL_MEAN)
            assert_allclose(mean, ref9["mean"], rtol=0, atol=ATOL_MEAN)
            kept[S] = out
        # a draw's bits do not depend on S or on the group it falls into
        assert np.array_equal(kept[1][0], kept[9][4])
        assert np.array_equal(kept[3], kept[9][:3])
        # null mean output: the same draws, bit for bit
        out0, _ = pathwise_call(_lib, H, P, blocks, shape, idx, y, Z9[:3], noiseless, want_mean=False)
        assert np.array_equal(out0, kept[3])
    print("%s: worst draws - oracle %.3e" % (pw_id(case), worst))


def test_pathwise_beyond_one_panel(eng):
    """The shapes of tests/test_gpu_pathwise.py::test_draws_beyond_one_panel: a 64 x 64 grid (prior blocks of 1024 points) with
    N = 1100 training points (nine 128-blocks: nine staging tiles of the cross apply, three outer panels of the solves).
    Same oracle, same bar; the dense host factors take seconds."""
    _lib, H = eng
    shape, N, Q, S = (64, 64), 1100, 4, 3
    P = params("narrow_u", Q, 2, 1)
    blocks = SSO.Blocks(PO.full_grid(shape)[0])                # (not cached: its basis change holds 128 MiB)
    M = blocks.M
    assert blocks.Nq == 1024 and blocks.B == 4
    idx = np.random.default_rng(N).permutation(M)[:N].astype(np.int64)
    X = blocks.G[idx]
    y = np.sin(X.sum(1) / 5.0) + 0.1 * np.random.default_rng(N + 1).standard_normal(N)
    cond = SSO.condition(P, blocks, idx)
    tol = draw_bar(P, cond)
    pm, _ = predict_sm(_lib, H, P, X, y, blocks.G)
    Z = np.random.default_rng(7).standard_normal((S, 2 * M + N))
    out, mean = pathwise_call(_lib, H, P, blocks, shape, idx, y, Z, 0)
    ref = SSO.draws(P, blocks, idx, y, Z, False)
    print("64x64-N1100-Q4-narrow_u S=3: draws - oracle %.3e (bar %.3e, cond %.3e, sum w %.3g), mean - predict %.3e, "
          "mean - oracle %.3e" % (np.abs(out - ref["out"]).max(), tol, cond, P.var, np.abs(mean - pm).max(),
                                  np.abs(mean - ref["mean"]).max()))
    assert np.isfinite(out).all()
    assert_allclose(out, ref["out"], rtol=0, atol=tol)
    assert_allclose(mean, pm, rtol=0, atol=ATOL_MEAN)
    assert_allclose(mean, ref["mean"], rtol=0, atol=ATOL_MEAN)
    # a draw's bits do not depend on S at these orders either
    one, _ = pathwise_call(_lib, H, P, blocks, shape, idx, y, Z[1:2], 0, want_mean=False)
    assert np.array_equal(one[0], out[1])


# ---------------------------------------------------------------------------------------------- joint through the C ABI
def joint_call(_lib, H, P, X, y, Xs, Z, noiseless, jitter=JITTER, want_moments=True):
    sm = sm_struct(_lib, X.shape[1], P.Q, P.D)
    S, M, N = Z.shape[0], len(Xs), len(X)
    Xd, yd, ud, Sd, Zd = dev(X), dev(y), dev(P.u), dev(Xs), dev(Z)
    out = torch.full((S, M), float("nan"), dtype=torch.float64, device="cuda")
    mean = torch.full((M,), float("nan"), dtype=torch.float64, device="cuda") if want_moments else None
    var = torch.full((M,), float("nan"), dtype=torch.float64, device="cuda") if want_moments else None
    _lib.check(H.lib.gpimhip_sample_sm(H.h, ctypes.byref(sm), _lib.ptr(Xd), _lib.ptr(yd), N, _lib.ptr(ud), _lib.ptr(Sd), M,
                                       _lib.ptr(Zd), S, int(noiseless), float(jitter), _lib.ptr(mean), _lib.ptr(var),
                                       _lib.ptr(out)))
    if not want_moments:
        return out.cpu().numpy(), None, None
    return out.cpu().numpy(), mean.cpu().numpy(), var.cpu().numpy()


JOINT_CASES = tuple((N, M, d, gen, noiseless) for (N, M, d) in ((100, 1, 2), (100, 77, 3), (256, 128, 2), (300, 129, 3))
                    for gen in ("random_u", "narrow_u") for noiseless in (0, 1))


@pytest.mark.parametrize("case", JOINT_CASES, ids=lambda c: "N%d-M%d-d%d-%s-%s" % (c[0], c[1], c[2], c[3], "noiseless" if c[4] else "noisy"))
def test_joint_against_oracle(eng, case):
    _lib, H = eng
    N, M, d, gen, noiseless = case
    Q = 3
    P = params(gen, Q, d, 1)
    X, y = SO.random_data(N, d, N)
    Xs = np.random.default_rng(11).uniform(0.0, 8.0, size=(M, d))
    Z9 = np.random.default_rng(100 + noiseless).standard_normal((9, M))
    ref = SSO.joint_draws(P, X, y, Xs, Z9, noiseless)
    # the explicit factor: out - mean = L22 z
    L = SSO.joint_factor(P, X, Xs, noiseless)
    assert np.abs(ref["out"] - (ref["mean"][None, :] + Z9 @ L[N:, N:].T)).max() <= 1e-12 * P.var
    tol = draw_bar(P, ref["cond"])
    mean_o, var_o = SO.predict(P.u, X, y, Xs, Q, d)
    pm, pv = predict_sm(_lib, H, P, X, y, Xs)
    kept = {}
    for S in (9, 1):
        rows = slice(4, 5) if S == 1 else slice(0, S)
        out, mean, var = joint_call(_lib, H, P, X, y, Xs, Z9[rows], noiseless)
        print("joint N=%d M=%d d=%d %s noiseless=%d S=%d: draws - oracle %.3e (bar %.3e, cond %.3e, sum w %.3g), mean - oracle "
              "%.3e, mean - predict %.3e, var - oracle %.3e, var - predict %.3e (bar %.3e)"
              % (N, M, d, gen, noiseless, S, np.abs(out - ref["out"][rows]).max(), tol, ref["cond"], P.var,
                 np.abs(mean - mean_o).max(), np.abs(mean - pm).max(), np.abs(var - var_o).max(), np.abs(var - pv).max(),
                 1e-10 * P.var))
        assert np.isfinite(out).all()
        assert_allclose(out, ref["out"][rows], rtol=0, atol=tol)
        assert_allclose(mean, mean_o, rtol=0, atol=ATOL_MEAN)
        assert_allclose(mean, pm, rtol=0, atol=ATOL_MEAN)
        assert_allclose(var, var_o, rtol=0, atol=1e-10 * P.var)
        assert_allclose(var, pv, rtol=0, atol=1e-10 * P.var)
        kept[S] = out
    assert np.array_equal(kept[1][0], kept[9][4])
    out0, _, _ = joint_call(_lib, H, P, X, y, Xs, Z9, noiseless, want_moments=False)
    assert np.array_equal(out0, kept[9])


# ---------------------------------------------------------------------------------------------- blocks through the C ABI
def blocks_call(_lib, H, P, blocks, shape, y, Z, noiseless, jitter=JITTER, want_mean=True):
    sm = sm_struct(_lib, len(shape), P.Q, P.D)
    S, M = Z.shape[0], blocks.M
    Gd, yd, ud, Zd = dev(blocks.G), dev(y), dev(P.u), dev(Z)
    out = torch.full((S, M), float("nan"), dtype=torch.float64, device="cuda")
    mean = torch.full((M,), float("nan"), dtype=torch.float64, device="cuda") if want_mean else None
    _lib.check(H.lib.gpimhip_sample_sm_blocks(H.h, ctypes.byref(sm), _lib.ptr(Gd), *grid_args(blocks, shape), _lib.ptr(yd),
                                              _lib.ptr(ud), _lib.ptr(Zd), S, int(noiseless), float(jitter), _lib.ptr(mean),
                                              _lib.ptr(out)))
    return out.cpu().numpy(), (mean.cpu().numpy() if want_mean else None)


BLOCK_CASES = tuple((shape, Q, iso, gen) for (shape, Q, iso) in (((6, 5), 3, False), ((24, 24), 4, False), ((4, 3, 4), 2, True))
                    for gen in ("random_u", "narrow_u"))


@pytest.mark.parametrize("case", BLOCK_CASES, ids=lambda c: "%s-Q%d-%s" % ("x".join(str(n) for n in c[0]), c[1], c[3]))
def test_blocks_against_oracle(eng, case):
    """Fully observed grids: the entry takes y in grid order; rows in a permuted order go through the Python surface, whose
    host layer puts them in grid order (a model built from a list of points: rec.solver == 'dense')."""
    import gpim_amd
    _lib, H = eng
    shape, Q, iso, gen = case
    d = len(shape)
    P = params(gen, Q, 1 if iso else d, 1)
    blocks = blocks_of(shape)
    M = blocks.M
    y = np.sin(blocks.G.sum(1) / 5.0) + 0.1 * np.random.default_rng(M).standard_normal(M)
    pm, _ = predict_sm(_lib, H, P, blocks.G, y, blocks.G)
    for noiseless in (1, 0):
        Z9 = np.random.default_rng(200 + noiseless).standard_normal((9, (2 if noiseless else 3) * M))
        ref = SSO.blocks_draws(P, blocks, y, Z9, noiseless)
        tol = draw_bar(P, ref["cond"])
        kept = {}
        for S in (9, 3, 1):
            rows = slice(4, 5) if S == 1 else slice(0, S)
            out, mean = blocks_call(_lib, H, P, blocks, shape, y, Z9[rows], noiseless)
            print("blocks %s noiseless=%d S=%d: draws - oracle %.3e (bar %.3e, cond %.3e, sum w %.3g), mean - predict %.3e, "
                  "mean - oracle %.3e" % (case, noiseless, S, np.abs(out - ref["out"][rows]).max(), tol, ref["cond"], P.var,
                                          np.abs(mean - pm).max(), np.abs(mean - ref["mean"]).max()))
            assert np.isfinite(out).all()
            assert_allclose(out, ref["out"][rows], rtol=0, atol=tol)
            assert_allclose(mean, pm, rtol=0, atol=ATOL_MEAN)
            assert_allclose(mean, ref["mean"], rtol=0, atol=ATOL_MEAN)
            kept[S] = out
        assert np.array_equal(kept[1][0], kept[9][4])
        assert np.array_equal(kept[3], kept[9][:3])
        out0, _ = blocks_call(_lib, H, P, blocks, shape, y, Z9[:3], noiseless, want_mean=False)
        assert np.array_equal(out0, kept[3])
        # the same observations as a list of points in a permuted order: z_e stays indexed by the grid point
        perm = np.random.default_rng(5).permutation(M)
        Xg, _ = PO.full_grid(shape)
        rec = gpim_amd.skreconstructor(blocks.G[perm].T.copy(), y[perm], Xg, kernel='Spectral', n_mixtures=Q, isotropic=iso,
                                       verbose=0)
        assert rec.solver == "dense"
        rec._u.copy_(dev(P.u))
        outp = rec.sample(3, z=Z9[:3], noiseless=bool(noiseless), method='blocks')
        assert outp.shape == (3,) + shape
        assert np.array_equal(outp.reshape(3, M), kept[3])


# ---------------------------------------------------------------------------------------------- the Python surface
def spectral(X, y, Xtest=None, Q=3, **kw):
    import gpim_amd
    return gpim_amd.skreconstructor(X, y, Xtest, kernel='Spectral', n_mixtures=Q, verbose=0, **kw)


def lattice(shape, seed):
    ii, jj = np.meshgrid(*[np.arange(float(n)) for n in shape], indexing="ij")
    return np.cos(2 * np.pi * ii / 5.0) * np.cos(2 * np.pi * jj / 4.0) + 0.05 * np.random.default_rng(seed).standard_normal(shape)


def untouched(rec, before):
    Xt, fd = before
    same = (rec.Xtest is None and Xt is None) or (rec.Xtest is not None and Xt is not None and rec.Xtest is Xt)
    return same and tuple(rec.fulldims) == fd


def state(rec):
    return rec.Xtest, tuple(rec.fulldims)


def check_surface(rec, methods, N, shape, Xg):
    """Shape, purity in z, seeding, and the antithetic mean for each method of `methods` on the grid Xg (N observations)."""
    M = int(np.prod(shape))
    mean_p, _ = rec.predict(Xg)
    for method in methods:
        W = {"joint": M, "pathwise": M + N, "blocks": 2 * M}[method]
        z = np.random.default_rng(3).standard_normal((2, W))
        a = rec.sample(2, Xg, noiseless=True, z=z, method=method)
        b = rec.sample(2, Xg, noiseless=True, z=z, method=method)
        assert a.shape == (2,) + shape and np.array_equal(a, b)
        s1 = rec.sample(2, seed=7, method=method)
        s2 = rec.sample(2, seed=7, method=method)
        s3 = rec.sample(2, seed=8, method=method)
        assert s1.shape == (2,) + shape and np.array_equal(s1, s2) and not np.array_equal(s1, s3)
        # z and -z average to the mean exactly, to rounding: the draws are affine in z
        m = rec.sample(2, noiseless=True, z=-z, method=method)
        scale = np.abs(a).max() + np.abs(mean_p).max()
        print("%s %s: |(f(z) + f(-z)) / 2 - mean| %.3e" % (rec.solver, method, np.abs(0.5 * (a + m) - mean_p[None]).max()))
        assert np.abs(0.5 * (a + m) - mean_p[None]).max() <= ATOL_MEAN * max(1.0, scale)


def test_surface_complete_image():
    shape = (16, 16)
    R = lattice(shape, 1)
    Xg, _ = PO.full_grid(shape)
    rec = spectral(Xg, R, Xg)
    assert rec.solver == "reflection"
    rec.train(iterations=3)
    check_surface(rec, ("joint", "pathwise", "blocks"), R.size, shape, Xg)
    M = 256
    before = state(rec)
    with pytest.raises(ValueError, match="z must have shape"):
        rec.sample(2, z=np.zeros((2, M + 1)), method='joint')
    with pytest.raises(ValueError, match="z must have shape"):
        rec.sample(2, z=np.zeros((3, 3 * M)), method='blocks')
    noise = rec._params()[4]
    for method, bad in (("pathwise", 0.0), ("pathwise", 1.01 * noise), ("blocks", -1e-6), ("blocks", 1.01 * noise), ("joint", -1e-9)):
        with pytest.raises(ValueError, match="jitter"):
            rec.sample(1, jitter=bad, method=method)
    for method in ("border", "kron", "columns"):
        with pytest.raises(NotImplementedError, match="'joint'.*'pathwise'.*'blocks'"):
            rec.sample(1, method=method)
    with pytest.raises(ValueError, match="method must be"):
        rec.sample(1, method="nystrom")
    bad = Xg.copy()
    bad[0, 3, 3] = np.nan
    for method in ("joint", "pathwise", "blocks"):
        with pytest.raises(ValueError, match="finite"):
            rec.sample(1, bad, method=method)
    # a grid that is not the training grid: 'blocks' refuses, and nothing is stored
    Xo = PO.full_grid((16, 14))[0]
    with pytest.raises(NotImplementedError):
        rec.sample(1, Xo, method='blocks')
    assert untouched(rec, before)
    # jitter == noise is allowed (the rule's upper end)
    assert np.isfinite(rec.sample(1, jitter=noise, method='blocks')).all()


def test_surface_image_with_missing_pixels():
    shape = (16, 16)
    R = lattice(shape, 2)
    hole = np.random.default_rng(9).permutation(R.size)[:13]
    R.reshape(-1)[hole] = np.nan
    Xg, _ = PO.full_grid(shape)
    Xh = Xg.copy()
    Xh[:, np.isnan(R)] = np.nan
    rec = spectral(Xh, R, Xg)
    assert rec.solver == "border"
    rec.train(iterations=3)
    obs = ~np.isnan(R.ravel())
    check_surface(rec, ("pathwise", "joint"), int(obs.sum()), shape, Xg)
    # a draw fills the holes, and equals the oracle's on the same normals
    u = rec._u.cpu().numpy()
    P = SSO.Params(u, 3, 2)
    blocks = blocks_of(shape)
    idx = np.flatnonzero(obs).astype(np.int64)
    Z = np.random.default_rng(4).standard_normal((3, 2 * 256 + len(idx)))
    out = rec.sample(3, z=Z, method='pathwise')
    ref = SSO.draws(P, blocks, idx, R.ravel()[obs], Z, False)
    cond = SSO.condition(P, blocks, idx)
    assert np.isfinite(out).all()
    assert_allclose(out.reshape(3, -1), ref["out"], rtol=0, atol=draw_bar(P, cond))
    before = state(rec)
    with pytest.raises(NotImplementedError, match="observation on every point"):
        rec.sample(1, method='blocks')
    with pytest.raises(NotImplementedError, match="'joint'.*'pathwise'.*'blocks'"):
        rec.sample(1, method='border')
    assert untouched(rec, before)
    # the same model forced dense draws the same
    rd = spectral(Xh, R, Xg, solver='dense')
    assert rd.solver == "dense"
    rd._u.copy_(rec._u)
    assert np.array_equal(rd.sample(3, z=Z, method='pathwise'), out)


def test_surface_scattered_points():
    X, y = SO.grid_data(60, 16, 3)
    Xg, _ = PO.full_grid((16, 16))
    rec = spectral(X.T.copy(), y, Xg)
    assert rec.solver == "dense"
    rec.train(iterations=3)
    check_surface(rec, ("joint", "pathwise"), len(X), (16, 16), Xg)
    before = state(rec)
    with pytest.raises(NotImplementedError, match="observation on every point"):
        rec.sample(1, method='blocks')
    with pytest.raises(ValueError, match="z must have shape"):
        rec.sample(1, z=np.zeros((1, 256)), method='pathwise')
    # scattered test rows off the grid: 'joint' serves them, 'pathwise' refuses
    Xs = np.random.default_rng(1).uniform(0, 15, size=(2, 37))
    with pytest.raises(NotImplementedError):
        rec.sample(1, Xs, method='pathwise')
    assert untouched(rec, before)
    assert rec.sample(2, Xs, seed=1).shape == (2, 37)
    assert tuple(rec.fulldims) == (37,)


def test_precision_single_stays_refused():
    Xg, _ = PO.full_grid((6, 5))
    with pytest.raises(NotImplementedError, match="single"):
        spectral(Xg, np.zeros((6, 5)), precision="single")
