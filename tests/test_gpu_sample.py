"""
Joint posterior draws on the MI355X: gpimhip_sample_exact against the explicit float64 route of the oracle
(tests/sample_oracle.py), reconstructor.sample and boptimizer(acquisition_function='ts').

Every bar is atol 1e-10, the bar tests/test_gpu_ops.py holds the posterior mean and variance to: two independent float64
routes on the CPU agree to 1.7e-12 or better on these inputs (tests/test_sample_host.py), which leaves ~50x room.
"""
import ctypes

import numpy as np
import pytest
import torch
from numpy.testing import assert_allclose

pytestmark = pytest.mark.gpu

import sample_oracle as SO

ATOL = 1e-10


@pytest.fixture(scope="module")
def eng(ensure_built):
    from gpim_amd import _lib
    H = _lib.Handle()
    yield _lib, H
    H.close()


def dev(t):
    return t.cuda().contiguous()


def sample_call(_lib, H, m, Xd, yd, ud, Xsd, Z, noiseless, jitter=SO.JITTER, want_moments=True):
    """gpimhip_sample_exact -> (samples (S, M), mean, var) on the host (mean / var None when not asked for)"""
    S, M = Z.shape
    Zd = dev(Z)
    out = torch.full((S, M), float("nan"), dtype=torch.float64, device="cuda")
    mean = torch.full((M,), float("nan"), dtype=torch.float64, device="cuda") if want_moments else None
    var = torch.full((M,), float("nan"), dtype=torch.float64, device="cuda") if want_moments else None
    _lib.check(H.lib.gpimhip_sample_exact(H.h, ctypes.byref(m), _lib.ptr(Xd), _lib.ptr(yd), Xd.shape[0], _lib.ptr(ud),
                                          _lib.ptr(Xsd), M, _lib.ptr(Zd), S, int(noiseless), float(jitter),
                                          _lib.ptr(mean), _lib.ptr(var), _lib.ptr(out)))
    return out.cpu(), (mean.cpu() if want_moments else None), (var.cpu() if want_moments else None)


@pytest.mark.parametrize("case", SO.CASES, ids=SO.case_id)
def test_sample_exact(eng, case):
    _lib, H = eng
    kind, N, M, d, how, noiseless = case
    R = SO.reference(case)
    m = R["spec"].struct()
    Xd, yd, ud, Xsd = dev(R["X"]), dev(R["y"]), dev(R["u"]), dev(R["Xs"])
    # --- the factor: S = M draws with Z = I give the columns of chol(Sigma)
    smp, mean, var = sample_call(_lib, H, m, Xd, yd, ud, Xsd, torch.eye(M, dtype=torch.float64), noiseless)
    D = (smp - mean[None, :]).t().contiguous()                  # D[i, s] = samples[s, i] - mean[i]
    print("factor: upper %.3e, D D^T - Sigma %.3e, D - L_ref %.3e" % (
        torch.triu(D, 1).abs().max().item() if M > 1 else 0.0, (D @ D.t() - R["Sigma"]).abs().max().item(),
        (D - R["L"]).abs().max().item()))
    assert_allclose(torch.triu(D, 1).numpy(), 0.0, rtol=0, atol=ATOL)
    assert_allclose((D @ D.t()).numpy(), R["Sigma"].numpy(), rtol=0, atol=ATOL)
    # --- mean and variance: gpimhip_predict_exact on the same handle, and the oracle
    pm = torch.empty(M, dtype=torch.float64, device="cuda")
    pv = torch.empty_like(pm)
    _lib.check(H.lib.gpimhip_predict_exact(H.h, ctypes.byref(m), _lib.ptr(Xd), _lib.ptr(yd), N, _lib.ptr(ud),
                                           _lib.ptr(Xsd), M, _lib.ptr(pm), _lib.ptr(pv)))
    m_ref, v_ref = SO.O.ExactGP(R["X"], R["y"], R["kp"], SO.JITTER).predict(R["Xs"])
    print("mean - predict %.3e, mean - oracle %.3e, var - predict %.3e, var - oracle %.3e" % (
        (mean - pm.cpu()).abs().max().item(), (mean - m_ref).abs().max().item(), (var - pv.cpu()).abs().max().item(),
        (var - v_ref).abs().max().item()))
    assert_allclose(mean.numpy(), pm.cpu().numpy(), rtol=0, atol=ATOL)
    assert_allclose(var.numpy(), pv.cpu().numpy(), rtol=0, atol=ATOL)
    assert_allclose(mean.numpy(), m_ref.numpy(), rtol=0, atol=ATOL)
    assert_allclose(var.numpy(), v_ref.numpy(), rtol=0, atol=ATOL)
    # --- draws: seeded Z, the group sizes of the kernel (1; below a group; two full groups; a group and a tail)
    for S in (1, 3, 16, 17):
        Z = torch.randn(S, M, dtype=torch.float64, generator=torch.Generator().manual_seed(100 + S))
        smp, mean_s, var_s = sample_call(_lib, H, m, Xd, yd, ud, Xsd, Z, noiseless)
        own = mean[None, :] + Z @ D.t()
        ref = R["mean"][None, :] + Z @ R["L"].t()
        print("S = %d: draws - (mean + D Z) %.3e, draws - reference %.3e" % (
            S, (smp - own).abs().max().item(), (smp - ref).abs().max().item()))
        assert_allclose(smp.numpy(), own.numpy(), rtol=0, atol=ATOL)
        assert_allclose(smp.numpy(), ref.numpy(), rtol=0, atol=ATOL)
        assert torch.equal(mean_s, mean) and torch.equal(var_s, var)
        # --- null outputs: the same draws, bit for bit
        if S == 17:
            smp0, _, _ = sample_call(_lib, H, m, Xd, yd, ud, Xsd, Z, noiseless, want_moments=False)
            assert torch.equal(smp0, smp)


def test_bad_arguments(eng):
    _lib, H = eng
    R = SO.reference(SO.CASES[2])
    m = R["spec"].struct()
    Xd, yd, ud, Xsd = dev(R["X"]), dev(R["y"]), dev(R["u"]), dev(R["Xs"])
    M = Xsd.shape[0]
    Zd = torch.zeros(1, M, dtype=torch.float64, device="cuda")
    out = torch.empty_like(Zd)
    p = _lib.ptr

    def rc(X=Xd, y=yd, u=ud, Xs=Xsd, Mv=M, Z=Zd, S=1, jitter=1e-5, o=out):
        return H.lib.gpimhip_sample_exact(H.h, ctypes.byref(m), p(X), p(y), Xd.shape[0], p(u), p(Xs), Mv, p(Z), S, 0, jitter,
                                          None, None, p(o))
    assert rc() == _lib.OK
    for bad in (dict(X=None), dict(y=None), dict(u=None), dict(Xs=None), dict(Z=None), dict(o=None), dict(S=0), dict(Mv=0),
                dict(jitter=-1e-9), dict(jitter=float("nan"))):
        assert rc(**bad) == _lib.E_BADARG, bad
    H32 = _lib.Handle(precision="single")
    try:
        assert H32.lib.gpimhip_sample_exact(H32.h, ctypes.byref(m), p(Xd), p(yd), Xd.shape[0], p(ud), p(Xsd), M, p(Zd), 1, 0,
                                            1e-5, None, None, p(out)) == _lib.E_BADARG
    finally:
        H32.close()


def test_nothing_else_moves(ensure_built):
    """A draw uses a matrix of its own: the workspace of fit / predict keeps its contents and its size."""
    from gpim_amd import _lib
    R = SO.reference(("Matern52", 300, 129, 3, "random", 0))
    m, spec = R["spec"].struct(), R["spec"]
    Xd, yd, Xsd = dev(R["X"]), dev(R["y"]), dev(R["Xs"])
    N, M, T = Xd.shape[0], Xsd.shape[0], 5
    Z = torch.randn(3, M, dtype=torch.float64, generator=torch.Generator().manual_seed(1))

    def predict(H, ud):
        pm = torch.empty(M, dtype=torch.float64, device="cuda")
        pv = torch.empty_like(pm)
        _lib.check(H.lib.gpimhip_predict_exact(H.h, ctypes.byref(m), _lib.ptr(Xd), _lib.ptr(yd), N, _lib.ptr(ud),
                                               _lib.ptr(Xsd), M, _lib.ptr(pm), _lib.ptr(pv)))
        return pm.cpu(), pv.cpu()

    def fit(H):
        ud = dev(R["u"].clone())
        hist = torch.empty(T, spec.n_params, dtype=torch.float64, device="cuda")
        loss = torch.empty(T, dtype=torch.float64, device="cuda")
        _lib.check(H.lib.gpimhip_fit_exact(H.h, ctypes.byref(m), _lib.ptr(Xd), _lib.ptr(yd), N, _lib.ptr(ud), 0.05, T,
                                           _lib.ptr(hist), _lib.ptr(loss)))
        return hist.cpu(), loss.cpu(), ud.cpu()

    H, H2 = _lib.Handle(), _lib.Handle()
    try:
        ud = dev(R["u"])
        before = predict(H, ud)
        bytes0 = H.lib.gpimhip_workspace_bytes(H.h)
        s1 = sample_call(_lib, H, m, Xd, yd, ud, Xsd, Z, 0)
        bytes1 = H.lib.gpimhip_workspace_bytes(H.h)
        s2 = sample_call(_lib, H, m, Xd, yd, ud, Xsd, Z, 0)
        bytes2 = H.lib.gpimhip_workspace_bytes(H.h)
        assert bytes1 > bytes0 and bytes2 == bytes1             # counted, and no growth at the same sizes
        assert all(torch.equal(a, b) for a, b in zip(s1, s2))
        # a smaller order afterwards re-uses the matrix
        sample_call(_lib, H, m, Xd, yd, ud, Xsd[:40].contiguous(), Z[:, :40].contiguous(), 0)
        assert H.lib.gpimhip_workspace_bytes(H.h) <= bytes2
        after = predict(H, ud)
        assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
        got, fresh = fit(H), fit(H2)
        assert all(torch.equal(a, b) for a, b in zip(got, fresh))
    finally:
        H.close()
        H2.close()


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


def test_reconstructor_sample(fitted):
    gpim_amd, r, R = fitted
    from gpim_amd import _lib
    a = r.sample(n_samples=3, seed=1)
    assert a.shape == (3, 16, 16) and a.dtype == np.float64 and np.isfinite(a).all()
    assert np.array_equal(a, r.sample(n_samples=3, seed=1))
    assert not np.array_equal(a, r.sample(n_samples=3, seed=2))
    assert r.sample().shape == (1, 16, 16)
    # the documented rule for the implicit draw
    M = 256
    g = torch.Generator(r._dev).manual_seed(1)
    z = torch.randn((3, M), dtype=torch.float64, device=r._dev, generator=g)
    assert np.array_equal(a, r.sample(n_samples=3, z=z))
    assert np.array_equal(a, r.sample(n_samples=3, z=z.cpu().numpy()))
    torch.cuda.manual_seed(5)
    b = r.sample(n_samples=2)
    torch.cuda.manual_seed(5)
    zb = torch.randn((2, M), dtype=torch.float64, device=r._dev)
    assert np.array_equal(b, r.sample(n_samples=2, z=zb))
    # z given: the C ABI's result
    for noiseless in (False, True):
        smp, mean, var = sample_call(_lib, r._handle, r._mstruct, r._Xd, r._yd, r._u, r._Xtest_d, z.cpu(), noiseless,
                                     jitter=r._spec.jitter)
        assert np.array_equal(r.sample(n_samples=3, z=z, noiseless=noiseless), smp.numpy().reshape(3, 16, 16))
    pm, psd = r.predict(verbose=0)
    assert_allclose(mean.numpy().reshape(16, 16), pm, rtol=0, atol=ATOL)
    assert_allclose(var.sqrt().numpy().reshape(16, 16), psd, rtol=0, atol=ATOL)
    with pytest.raises(ValueError):
        r.sample(n_samples=2, z=z)
    # a test grid with a NaN row
    Xnan = gpim_amd.utils.get_full_grid(R).astype(np.float64)
    Xnan[:, 3, 4] = np.nan
    with pytest.raises(ValueError):
        r.sample(Xtest=Xnan)
    assert np.array_equal(a, r.sample(n_samples=3, seed=1))     # the refused grid did not replace the stored one


def test_sample_refused_off_the_dense_double_engine(fitted):
    gpim_amd, _, R = fitted
    Xs, Xf = gpim_amd.utils.get_sparse_grid(R), gpim_amd.utils.get_full_grid(R)
    _, full = image16()
    models = [gpim_amd.reconstructor(Xs, R, Xf, sparse=True, indpoints=20, iterations=1, verbose=0),
              gpim_amd.reconstructor(Xf, full, Xf, structured=True, iterations=1, verbose=0),
              gpim_amd.reconstructor(Xf, full, Xf, kernel="Matern52", structured=True, iterations=1, verbose=0),
              gpim_amd.reconstructor(Xs, R, Xf, precision="single", iterations=1, verbose=0)]
    for model in models:
        with pytest.raises(NotImplementedError, match="dense double-precision engine"):
            model.sample()


def model_of(gpim_amd, method):
    """(the smallest model that reaches `method`, the Xtest of the call): 8 x 8 images, an 8 x 7 x 5 cube for 'columns'"""
    from columns_oracle import cube
    rng = np.random.default_rng(0)
    ii, jj = np.meshgrid(np.arange(8.0), np.arange(8.0), indexing="ij")
    full = np.cos(ii / 3.0) * np.sin(jj / 2.0 + 0.3) + 0.05 * rng.standard_normal((8, 8))
    Xf = gpim_amd.utils.get_full_grid(full)
    kw = dict(lengthscale=[[1., 1.], [6., 6.]], iterations=1, verbose=0)
    if method in ("joint", "pathwise"):             # 40 scattered observations; off the grid for 'joint'
        R = full.copy()
        R.ravel()[rng.permutation(64)[:24]] = np.nan
        Xs = gpim_amd.utils.get_sparse_grid(R)
        if method == "joint":
            Xs = Xs + np.where(np.isnan(Xs), 0.0, 0.3 * rng.random(Xs.shape))
        return gpim_amd.reconstructor(Xs, R, Xf, kernel="RBF", **kw), None
    if method == "blocks":
        return gpim_amd.reconstructor(Xf, full, Xf, kernel="Matern52", structured=True, **kw), None
    if method == "kron":                            # drawn on a grid twice as fine
        return (gpim_amd.reconstructor(Xf, full, Xf, kernel="RBF", structured=True, **kw),
                gpim_amd.utils.get_full_grid(full, dense_x=0.5))
    if method == "border":                          # 5 scattered pixels missing
        R = full.copy()
        for p in ((1, 2), (3, 5), (4, 1), (6, 6), (2, 4)):
            R[p] = np.nan
        Xs = gpim_amd.utils.get_sparse_grid(R)
        return gpim_amd.reconstructor(Xs, R, Xf, kernel="Matern52", structured=True,
                                      _border=gpim_amd.utils.border_blocks(Xs, R), **kw), None
    Xg, Xc, Rc = cube((8, 7, 5), (0, 1), 0.6, seed=0)       # 40 % of the pixels observed
    rec = gpim_amd.skreconstructor(Xc, Rc, Xg, kernel="RBF", lengthscale=[[0.1] * 3, [100.0] * 3], verbose=0)
    assert rec.solver == "columns"
    return rec, None


@pytest.mark.parametrize("method", ("joint", "pathwise", "blocks", "border", "kron", "columns"))
def test_seeded_draw_is_the_documented_randn(ensure_built, method):
    """sample(seed=k) is sample(z=torch.randn((S, W), dtype=float64, device=dev, generator=Generator(dev).manual_seed(k))),
    bit for bit, with W the width the method's description plans: the position and the width of the implicit draw."""
    import gpim_amd
    from gpim_amd import _sampling
    rec, Xtest = model_of(gpim_amd, method)
    m = _sampling.METHODS[method]
    S, k = 2, 3
    for noiseless in (False, True):
        W = m.plan(m.geometry(rec, *m.grid(rec, Xtest)), S, noiseless, True)[0]
        z = torch.randn((S, W), dtype=torch.float64, device=rec._dev, generator=torch.Generator(rec._dev).manual_seed(k))
        a = rec.sample(n_samples=S, Xtest=Xtest, seed=k, noiseless=noiseless, method=method)
        b = rec.sample(n_samples=S, Xtest=Xtest, z=z, noiseless=noiseless, method=method)
        assert a.shape == (S,) + tuple(rec.fulldims) and np.isfinite(a).all() and a.std() > 0
        assert np.array_equal(a, b), (method, noiseless, W)
        # a z one column wider or narrower is refused: W is the only width
        for bad in (W - 1, W + 1):
            with pytest.raises(ValueError, match="z must have shape"):
                rec.sample(n_samples=S, Xtest=Xtest, z=np.zeros((S, bad)), noiseless=noiseless, method=method)


def bo_problem():
    rng = np.random.default_rng(4)
    ii, jj = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    Zt = np.exp(-((ii - 5) ** 2 + (jj - 11) ** 2) / 20.0) + 0.5 * np.exp(-((ii - 12) ** 2 + (jj - 3) ** 2) / 30.0)
    Z = np.full((16, 16), np.nan)
    idx = rng.permutation(256)[:20]
    Z.ravel()[idx] = Zt.ravel()[idx]
    return Zt, Z


def make_bo(gpim_amd, tmp_path, **kw):
    Zt, Z = bo_problem()
    return gpim_amd.boptimizer(gpim_amd.utils.get_sparse_grid(Z), Z.copy(), gpim_amd.utils.get_full_grid(Z),
                               lambda idx: Zt[tuple(idx)], acquisition_function="ts", exploration_steps=3,
                               gp_iterations=20, learning_rate=0.1, seed=3, verbose=0, filename=str(tmp_path / "bo"), **kw)


def test_boptimizer_thompson(fitted, tmp_path):
    gpim_amd = fitted[0]
    runs = []
    for _ in range(2):
        bo = make_bo(gpim_amd, tmp_path)
        bo.run()
        runs.append(bo)
    a, b = runs
    assert len(a.indices_all) == 3 and a.indices_all == b.indices_all
    assert len(a.gp_predictions) == 3
    # the first step on a second, identically built and trained optimiser: the draw by the documented rule
    c = make_bo(gpim_amd, tmp_path)
    sm = c.surrogate_model
    sm.train()
    M = 256
    z = torch.randn((1, M), dtype=torch.float64, device=sm._dev, generator=torch.Generator(sm._dev).manual_seed(3))
    draw = sm.sample(z=z, noiseless=True)[0]
    masked = np.where(np.isnan(bo_problem()[1]), draw, -np.inf)
    assert tuple(a.indices_all[0]) == tuple(int(v) for v in np.unravel_index(np.argmax(masked), masked.shape))
    pm, psd = sm.predict(verbose=0)
    assert_allclose(a.gp_predictions[0][0], pm, rtol=0, atol=ATOL)
    assert_allclose(a.gp_predictions[0][1], psd, rtol=0, atol=ATOL)
    # the public acquisition function: the same draw, mean and sd from the same call
    acq, (mean, sd) = gpim_amd.acqfunc.thompson_sampling(sm, c.X_full, z=z)
    assert np.array_equal(acq, draw)
    assert_allclose(mean, pm, rtol=0, atol=ATOL)
    assert_allclose(sd, psd, rtol=0, atol=ATOL)
    acq2, _ = gpim_amd.acqfunc.thompson_sampling(sm, c.X_full, seed=3)
    assert np.array_equal(acq2, draw)
    with pytest.raises(NotImplementedError):
        make_bo(gpim_amd, tmp_path, shard_candidates=True)
