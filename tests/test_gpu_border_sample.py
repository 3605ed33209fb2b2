"""
Posterior draws on a grid with missing points through the bordered reflection blocks on the MI355X:
gpimhip_sample_border and skreconstructor.sample(method='border') against the host oracle of tests/pathwise_oracle.py with
idx = the observed points, on the same standard normals -- device and oracle are both pure functions of z.

Bar of the draws: 10 x pathwise_oracle.HOST_DISCREPANCY x the condition number of the case, the largest among K_GG + s I on
the completed grid (it bounds K_oo + s I, a principal submatrix, and it is what the explicit inverses go through) and the
prior blocks K_b + d I.  The mean is held to gpimhip_predict_exact_batched on the same model at 1e-10 (the bar of
tests/test_gpu_blocks.py).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
from numpy.testing import assert_allclose

pytestmark = pytest.mark.gpu

import border_sample_oracle as BS
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


def block_condition(P, blocks, d):
    """border_sample_oracle.condition without an eigenvalue problem of the order of the grid: K_GG + s I is orthogonally
    similar to blockdiag(K_b + s I) on the rows that exist, so its extreme eigenvalues are the extremes over the blocks."""
    lo, hi, cb = np.inf, 0.0, 0.0
    for b, Kb in enumerate(blocks.prior_blocks(P, d)):
        pr = blocks.present[b]
        w = np.linalg.eigvalsh(Kb[np.ix_(pr, pr)])
        cb = max(cb, float(w[-1] / w[0]))
        lo, hi = min(lo, float(w[0]) + (P.s - d)), max(hi, float(w[-1]) + (P.s - d))
    return max(hi / lo, cb)


def problem(shape, kind, miss, blocks=None, pair=None):
    """One grid with the missing points `miss` (flat indices) and one model: parameters held identically by the oracle and the
    engine, the border form of the data (gprutils.border_blocks) on the device, the case's condition number."""
    from gpim_amd import _solvers, gprutils
    d = len(shape)
    kp, spec, u = pair if pair is not None else SO.pair(kind, d, [[1.0] * d, [6.0] * d], seed=3)
    P = PO.Params.from_oracle(kp, d, spec.jitter)
    blocks = blocks_of(tuple(shape)) if blocks is None else blocks
    M = blocks.M
    y = np.sin(blocks.G.sum(1) / 5.0) + 0.1 * np.random.default_rng(M + 1).standard_normal(M)
    miss = np.asarray(miss, dtype=np.int64)
    yn = y.copy()
    yn[miss] = np.nan
    Xg = PO.full_grid(shape)[0]
    Xn = Xg.copy()
    Xn.reshape(d, -1)[:, miss] = np.nan
    S = gprutils.border_blocks(Xn, yn.reshape(shape))
    assert np.array_equal(S["miss"], miss)
    S["n_total"] = S["n_obs"]
    D = _solvers.DeviceBlocks(S, torch.device("cuda"))
    D.upload_border()
    return dict(P=P, spec=spec, u=u, blocks=blocks, y=y, miss=miss, idx=np.flatnonzero(BS.observed(M, miss)), D=D, shape=tuple(shape),
                Gd=dev(blocks.G), miss_d=dev(miss), ud=dev(u).repeat(S["B"]).contiguous(), cond=None)


def tolerance(Q, d=SO.JITTER):
    if Q["cond"] is None:
        Q["cond"] = block_condition(Q["P"], Q["blocks"], d)
    return 10.0 * PO.HOST_DISCREPANCY * Q["cond"]


def border_rc(_lib, H, Q, Zd, noiseless, jitter, mean, out, mode="border", S=None, mask=None, miss="miss", B=None):
    D, m = Q["D"], Q["spec"].struct()
    shape = (ctypes.c_int32 * len(Q["shape"]))(*Q["shape"])
    call = lambda: H.lib.gpimhip_sample_border(
        H.h, ctypes.byref(m), _lib.ptr(D.Xq), 0, _lib.ptr(D.ys), D.Xq.shape[0], D.B if B is None else B, _lib.ptr(Q["ud"]),
        _lib.ptr(Q["Gd"]), shape, D.mask if mask is None else mask, D.twoc, ctypes.c_void_p(Q["miss_d"].data_ptr()) if miss else None, _lib.ptr(Zd),
        Zd.shape[0] if S is None else S, int(noiseless), float(jitter), _lib.ptr(mean), _lib.ptr(out))
    if mode == "dense":
        return call()
    with _lib.reflection(H, D, 0, D.border if mode == "border" else None):
        return call()


def border_call(_lib, H, Q, Z, noiseless, jitter=SO.JITTER, want_mean=True):
    """gpimhip_sample_border -> (samples (S, M), mean or None) on the host"""
    S, M = Z.shape[0], Q["blocks"].M
    out = torch.full((S, M), float("nan"), dtype=torch.float64, device="cuda")
    mean = torch.full((M,), float("nan"), dtype=torch.float64, device="cuda") if want_mean else None
    _lib.check(border_rc(_lib, H, Q, dev(Z), noiseless, jitter, mean, out))
    return out.cpu().numpy(), (mean.cpu().numpy() if want_mean else None)


def predict_mean(_lib, H, Q):
    """The posterior mean of the same border model on the completed grid (gpimhip_predict_exact_batched)."""
    D, m, M = Q["D"], Q["spec"].struct(), Q["blocks"].M
    pm = torch.empty(M, dtype=torch.float64, device="cuda")
    pv = torch.empty_like(pm)
    with _lib.reflection(H, D, 0, D.border):
        _lib.check(H.lib.gpimhip_predict_exact_batched(H.h, ctypes.byref(m), _lib.ptr(D.Xq), 0, _lib.ptr(D.ys), D.Xq.shape[0], D.B,
                                                       _lib.ptr(Q["ud"]), _lib.ptr(Q["Gd"]), M, _lib.ptr(pm), _lib.ptr(pv)))
    return pm.cpu().numpy()


def oracle(Q, Z, noiseless):
    Zp, idx = BS.pathwise_z(Z, Q["blocks"].M, Q["miss"])
    assert np.array_equal(idx, Q["idx"])
    return PO.draws(Q["P"], Q["blocks"], idx, Q["y"][idx], Zp, noiseless)


def check_case(_lib, H, Q, name, S, noiseless_set=(1, 0), seed=100):
    M = Q["blocks"].M
    tol = tolerance(Q)
    pm = predict_mean(_lib, H, Q)
    for noiseless in noiseless_set:
        Z = np.random.default_rng(seed + noiseless).standard_normal((S, 2 * M + (0 if noiseless else M)))
        out, mean = border_call(_lib, H, Q, Z, noiseless)
        ref = oracle(Q, Z, noiseless)
        print("%s noiseless=%d S=%d: draws - oracle %.3e (bar %.3e, cond %.3e), mean - predict %.3e, mean - oracle %.3e"
              % (name, noiseless, S, np.abs(out - ref["out"]).max(), tol, Q["cond"], np.abs(mean - pm).max(),
                 np.abs(mean - ref["mean"]).max()))
        assert np.isfinite(out).all()
        assert_allclose(out, ref["out"], rtol=0, atol=tol)
        assert_allclose(mean, pm, rtol=0, atol=ATOL_MEAN)
        assert_allclose(mean, ref["mean"], rtol=0, atol=ATOL_MEAN)
        # null mean output: the same draws, bit for bit; entries of z_e at the missing points are ignored
        Z2 = Z.copy()
        Z2[:, M + Q["miss"]] = 7.0
        out0, _ = border_call(_lib, H, Q, Z2, noiseless, want_mean=False)
        assert np.array_equal(out0, out)
    return Z, out, mean


def bit_checks(_lib, H, Q, noiseless):
    """Draw k of an S = 9 call (ten columns: a group of 8 and a group of 2 that carries y) is the S = 1 call on the same row of z
    (one group of 2), and S = 3 (a group of 4) and S = 6 (seven columns in the form for eight) reproduce their rows; the mean
    does not depend on the group that carries y."""
    M = Q["blocks"].M
    Z9 = np.random.default_rng(5 + noiseless).standard_normal((9, 2 * M + (0 if noiseless else M)))
    o9, m9 = border_call(_lib, H, Q, Z9, noiseless)
    o1, m1 = border_call(_lib, H, Q, Z9[4:5], noiseless)
    o3, m3 = border_call(_lib, H, Q, Z9[:3], noiseless)
    o6, m6 = border_call(_lib, H, Q, Z9[:6], noiseless)
    assert np.array_equal(o1[0], o9[4]) and np.array_equal(o3, o9[:3]) and np.array_equal(o6, o9[:6])
    assert np.array_equal(m1, m9) and np.array_equal(m3, m9) and np.array_equal(m6, m9)
    return Z9, o9, m9


# 6x5: one odd axis (a mirror plane and weights); 5x5: both odd (a stabiliser of four, blocks of different sizes); 8x8: no
# plane; 4x3x4: eight blocks.  Nq < 128 everywhere: one tile with identity padding.
GRIDS = ((6, 5), (5, 5), (8, 8), (4, 3, 4))
CASES = tuple((shape, kind) for shape in GRIDS for kind in SO.KINDS)


def case_id(c):
    return "%s-%s" % ("x".join(str(n) for n in c[0]), c[1])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_small_grids_against_oracle(eng, case):
    _lib, H = eng
    shape, kind = case
    for name, miss in BS.missing_sets(shape).items():
        Q = problem(shape, kind, miss)
        check_case(_lib, H, Q, "%s-%s" % (case_id(case), name), 3)


def missing_random(M, count, seed):
    return np.sort(np.random.default_rng(seed).choice(M, size=count, replace=False))


def test_two_tiles(eng):
    """24 x 24, 5 % missing: Nq = 144, so np = 256 (two tiles, the second mostly identity padding); mp = 128."""
    _lib, H = eng
    Q = problem((24, 24), "RationalQuadratic", missing_random(576, 29, 1))
    assert Q["D"].Xq.shape[0] == 144
    check_case(_lib, H, Q, "24x24-RationalQuadratic-5%", 3)
    for noiseless in (1, 0):
        bit_checks(_lib, H, Q, noiseless)


def test_beyond_one_panel(eng):
    """72 x 64, Matern52, noisy, S = 9, 150 missing points: Nq = np = 1152 (nine tiles, ld = np + 16, five row chunks of the
    transposed sweep, the forward sweep's interior chunks), mp = 256 (S spans two tiles); ten columns run as a group of 8 and a
    group of 2 that carries y.  Same oracle, same bar; the dense host factors of order 4458 take seconds."""
    _lib, H = eng
    shape = (72, 64)
    blocks = PO.Blocks(PO.full_grid(shape)[0])                # (not cached: its basis change holds 160 MiB)
    assert blocks.Nq == 1152 and blocks.B == 4
    Q = problem(shape, "Matern52", missing_random(blocks.M, 150, 2), blocks=blocks)
    Z9, o9, m9 = bit_checks(_lib, H, Q, 0)
    tol = tolerance(Q)
    ref = oracle(Q, Z9, False)
    pm = predict_mean(_lib, H, Q)
    print("72x64-Matern52 S=9: draws - oracle %.3e (bar %.3e, cond %.3e), mean - predict %.3e, mean - oracle %.3e"
          % (np.abs(o9 - ref["out"]).max(), tol, Q["cond"], np.abs(m9 - pm).max(), np.abs(m9 - ref["mean"]).max()))
    assert np.isfinite(o9).all()
    assert_allclose(o9, ref["out"], rtol=0, atol=tol)
    assert_allclose(m9, pm, rtol=0, atol=ATOL_MEAN)
    assert_allclose(m9, ref["mean"], rtol=0, atol=ATOL_MEAN)


def test_bad_arguments_workspace_and_failed_factorisation(eng):
    _lib, H = eng
    shape = (8, 8)
    Q = problem(shape, "Matern52", BS.missing_sets(shape)["random"])
    M = Q["blocks"].M
    Z = np.random.default_rng(9).standard_normal((2, 2 * M))
    a, am = border_call(_lib, H, Q, Z, 1)
    bytes1 = H.lib.gpimhip_workspace_bytes(H.h)
    b, _ = border_call(_lib, H, Q, Z, 1)
    assert H.lib.gpimhip_workspace_bytes(H.h) == bytes1 and np.array_equal(a, b)
    for bad in (0.0, -1e-9, float("nan")):
        with pytest.raises(ValueError):
            border_call(_lib, H, Q, Z, 1, jitter=bad)
    Zd = dev(Z)
    out = torch.empty((2, M), dtype=torch.float64, device="cuda")
    rc = lambda h=H, **kw: border_rc(_lib, h, Q, Zd, 1, 1e-5, None, kw.pop("o", out), **kw)
    assert rc() == _lib.OK
    # no draws, null pointers, a mask that is not the handle's
    for kw in (dict(S=0), dict(miss=None), dict(o=None), dict(mask=1), dict(mask=0)):
        assert rc(**kw) == _lib.E_BADARG, kw
    # no reflection mode; reflection mode without a border
    assert rc(mode="dense") == _lib.E_BADARG
    assert b"needs reflection mode" in H.lib.gpimhip_last_error()
    assert rc(mode="reflection") == _lib.E_BADARG
    assert b"no border is set" in H.lib.gpimhip_last_error()
    assert rc() == _lib.OK
    # a single-precision handle refuses reflection mode, and the entry itself outside it
    H32 = _lib.Handle(precision="single")
    try:
        assert rc(h=H32, mode="dense") == _lib.E_BADARG
        assert b"double-precision" in H.lib.gpimhip_last_error()
    finally:
        H32.close()
    # a failed factorisation: RBF with a lengthscale 40 x the grid and neither noise nor jitter to speak of -- the blocks are
    # numerically singular (numpy's Cholesky fails on them too); the handle stays usable and gives the same bits as before
    bad = SO.pair("RBF", 2, [[320.0, 320.0], [321.0, 321.0]], seed=3, jitter=1e-30, noise_u=-80.0)
    Qb = problem((16, 16), "RBF", [20, 70], pair=bad)
    with pytest.raises(np.linalg.LinAlgError):
        for Kb in Qb["blocks"].prior_blocks(Qb["P"], Qb["P"].s):
            np.linalg.cholesky(Kb)
    Zb = torch.zeros((2, 2 * 256), dtype=torch.float64, device="cuda")
    assert border_rc(_lib, H, Qb, Zb, 1, 1e-30, None, torch.empty((2, 256), dtype=torch.float64, device="cuda")) == _lib.E_NOT_PD
    assert b"not positive-definite" in H.lib.gpimhip_last_error()
    c, cm = border_call(_lib, H, Q, Z, 1)
    assert np.array_equal(c, a) and np.array_equal(cm, am)


def test_multi_output_batch_is_refused_and_stale_borders_do_not_matter(eng):
    """The entry takes the 2^r blocks of one model: a batch of T 2^r problems (what a multi-output border would be) is refused
    with its own message, whatever the handle ran before.  What a handle ran before does not matter either: after a
    multi-output border call (vreconstructor's border solver leaves BorderWs::T = 2 on its handle) the draw on that handle
    gives the bits of a handle that never saw one, and the multi-output model goes on working."""
    import gpim_amd
    from test_gpu_vgp_border import knock_out
    from test_gpu_vgp_refl import grid_stack
    _lib, H = eng
    shape = (8, 8)
    Q = problem(shape, "Matern52", BS.missing_sets(shape)["random"])
    M = Q["blocks"].M
    Z = np.random.default_rng(11).standard_normal((2, 2 * M))
    want, wmean = border_call(_lib, H, Q, Z, 1)
    out = torch.empty((2, M), dtype=torch.float64, device="cuda")
    for T in (2, 3):
        assert border_rc(_lib, H, Q, dev(Z), 1, 1e-5, None, out, B=T * Q["D"].B) == _lib.E_BADARG
        assert b"multi-output border" in H.lib.gpimhip_last_error()
    again, amean = border_call(_lib, H, Q, Z, 1)
    assert np.array_equal(again, want) and np.array_equal(amean, wmean)
    X, Y = grid_stack((16, 16), 2, seed=1)
    Xn, Yn, _ = knock_out(X, Y, 0.05, seed=2)
    rb = gpim_amd.vreconstructor(Xn, Yn, kernel="Matern52", lengthscale=[0.5, 2.5], verbose=0, solver="border")
    assert rb.solver == "border"
    l0, g0 = rb.nll_grad()
    got, gmean = border_call(_lib, rb._handle, Q, Z, 1)
    assert np.array_equal(got, want) and np.array_equal(gmean, wmean)
    assert border_rc(_lib, rb._handle, Q, dev(Z), 1, 1e-5, None, out, B=2 * Q["D"].B) == _lib.E_BADARG
    assert b"multi-output border" in H.lib.gpimhip_last_error()
    l1, g1 = rb.nll_grad()
    assert np.isfinite(l0) and l1 == l0 and np.array_equal(np.asarray(g0), np.asarray(g1))


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
    R = full.copy()
    R[3, 4] = R[9, 2] = np.nan
    Xf, Xs = gpim_amd.utils.get_full_grid(R), gpim_amd.utils.get_sparse_grid(R)
    kw = dict(kernel="Matern52", lengthscale=[[1., 1.], [8., 8.]], learning_rate=0.1, iterations=3, verbose=0)
    sk = gpim_amd.skreconstructor(Xs, R, Xf, **kw)
    assert sk.solver == "border" and sk.do_border
    sk.train()
    dn = gpim_amd.reconstructor(Xs, R, Xf, **kw)
    dn._u.copy_(sk._u)                  # the dense model of the same data at the same hyper-parameters
    return gpim_amd, sk, dn, full, R, Xf, Xs


def test_skreconstructor_sample_border(models):
    gpim_amd, sk, dn, full, R, Xf, Xs = models
    M = 256
    P, blocks = oracle_params(sk), blocks_of((16, 16))
    miss = np.flatnonzero(np.isnan(R).reshape(-1))
    idx = np.flatnonzero(BS.observed(M, miss))
    tol = 10.0 * PO.HOST_DISCREPANCY * block_condition(P, blocks, P.jitter)
    a = sk.sample(n_samples=3, seed=1, method="border")
    assert a.shape == (3, 16, 16) and a.dtype == np.float64 and np.isfinite(a).all()
    assert np.array_equal(a, sk.sample(n_samples=3, seed=1, method="border"))
    assert not np.array_equal(a, sk.sample(n_samples=3, seed=2, method="border"))
    assert sk.sample(method="border").shape == (1, 16, 16)
    assert np.array_equal(a, sk.sample(n_samples=3, seed=1, Xtest=Xf, method="border"))        # the completed grid, given
    mean, sd = sk.predict(verbose=0)
    for noiseless in (False, True):
        W = 2 * M + (0 if noiseless else M)
        z = torch.randn((3, W), dtype=torch.float64, device=sk._dev, generator=torch.Generator(sk._dev).manual_seed(1))
        got = sk.sample(n_samples=3, z=z, noiseless=noiseless, method="border")
        assert np.array_equal(got, sk.sample(n_samples=3, seed=1, noiseless=noiseless, method="border"))
        assert np.array_equal(got, sk.sample(n_samples=3, z=z.cpu().numpy(), noiseless=noiseless, method="border"))
        zp, idx2 = BS.pathwise_z(z.cpu().numpy(), M, miss)
        assert np.array_equal(idx, idx2)
        ref = PO.draws(P, blocks, idx, full.reshape(-1)[idx], zp, noiseless)["out"].reshape(3, 16, 16)
        pw = dn.sample(n_samples=3, z=zp, noiseless=noiseless, method="pathwise")
        print("skreconstructor.sample(border) noiseless=%d: draws - oracle %.3e, - dense pathwise %.3e (bar %.3e)"
              % (noiseless, np.abs(got - ref).max(), np.abs(got - pw).max(), tol))
        assert_allclose(got, ref, rtol=0, atol=tol)
        assert_allclose(got, pw, rtol=0, atol=tol)
        if noiseless:
            # at the observed pixels a noiseless draw stays within a few posterior standard deviations of the data
            obs = ~np.isnan(R)
            assert (np.abs(got - R[None])[:, obs] <= 6.0 * sd[obs][None]).all()
    # the model still predicts
    mean2, sd2 = sk.predict(verbose=0)
    assert np.array_equal(mean, mean2) and np.array_equal(sd, sd2)


def test_refusals(models):
    gpim_amd, sk, dn, full, R, Xf, Xs = models
    grid_before = (sk.Xtest, sk._Xtest_d, sk.fulldims)
    before = sk.sample(n_samples=1, seed=4, method="border")

    def unchanged():
        assert sk.Xtest is grid_before[0] and sk._Xtest_d is grid_before[1] and sk.fulldims == grid_before[2]
        assert np.array_equal(before, sk.sample(n_samples=1, seed=4, method="border"))

    with pytest.raises(ValueError, match="method must be .*'border'"):
        sk.sample(method="matheron")
    for bad in (10.0, 0.0, -1e-6):
        with pytest.raises(ValueError, match="jitter"):
            sk.sample(method="border", jitter=bad)
        unchanged()
    # a wrong width of z: the joint route's, the noiseless width for noisy draws, the pathwise route's
    for W in (256, 512, 2 * 256 + 254):
        with pytest.raises(ValueError, match="shape"):
            sk.sample(n_samples=1, z=np.zeros((1, W)), method="border")
    with pytest.raises(ValueError, match="shape"):
        sk.sample(n_samples=1, z=np.zeros((1, 768)), noiseless=True, method="border")
    unchanged()
    # a test grid that is not the completed training grid: moved by half a pixel, a finer grid, a grid with a NaN
    with pytest.raises(NotImplementedError, match="completed training grid"):
        sk.sample(Xtest=Xf + 0.5, method="border")
    fine = np.array(np.meshgrid(np.arange(0.0, 15.5, 0.5), np.arange(0.0, 15.5, 0.5), indexing="ij"))
    with pytest.raises(NotImplementedError, match="completed training grid"):
        sk.sample(Xtest=fine, method="border")
    Xnan = Xf.astype(np.float64)
    Xnan[:, 3, 4] = np.nan
    with pytest.raises(ValueError, match="finite"):
        sk.sample(Xtest=Xnan, method="border")
    unchanged()
    # the other methods keep their refusals of a border model
    with pytest.raises(NotImplementedError, match="fully observed grid"):
        sk.sample(method="blocks")
    with pytest.raises(NotImplementedError, match="dense double-precision engine"):
        sk.sample(method="pathwise")
    unchanged()
    # models without a border, each named its alternative
    kw = dict(kernel="Matern52", lengthscale=[[1., 1.], [8., 8.]], iterations=1, verbose=0)
    skf = gpim_amd.skreconstructor(Xf, full, Xf, **kw)
    assert skf.solver == "reflection"
    for model, why in ((skf, "use method='blocks'"),
                       (gpim_amd.reconstructor(Xf, full, Xf, structured=True, **kw), "use method='blocks'"),
                       (dn, "use method='pathwise'"),
                       (gpim_amd.reconstructor(Xs, R, Xf, sparse=True, indpoints=20, iterations=1, verbose=0), "sparse=True"),
                       (gpim_amd.reconstructor(Xs, R, Xf, precision="single", iterations=1, verbose=0), "precision='single'")):
        g0 = (model.Xtest, model._Xtest_d, model.fulldims)
        with pytest.raises(NotImplementedError, match=why):
            model.sample(method="border")
        assert model.Xtest is g0[0] and model._Xtest_d is g0[1] and model.fulldims == g0[2]
        m, _ = model.predict(verbose=0)
        assert np.isfinite(m).all()
    from gpim_amd import _solvers
    for cls in (_solvers.Dense, _solvers.Sparse, _solvers.Kron):
        with pytest.raises(NotImplementedError):
            cls.sample_border(None, None)
    unchanged()
