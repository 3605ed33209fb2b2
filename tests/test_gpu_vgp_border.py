"""vreconstructor's border solver (incomplete grids) on the MI355X against the dense engine on the
same observed rows and parameters.  Every parity, training and repeatability case forces ``solver='border'`` (and the other
side ``solver='dense'``), so that none of them depends on the measured floor VGP_BORDER_MIN_OBS; only test_solver_choice
leaves the choice to the data."""
import ctypes

import numpy as np
import pytest
import torch

import vgp_oracle as V
from problems import spiral_image
from test_gpu_vgp import eels_twin, scattered
from test_gpu_vgp_refl import chunked_predict, grid_stack

pytestmark = pytest.mark.gpu


def knock_out(X, Y, missing, seed):
    """Copies of X (d, *shape) and Y (*shape, T) with NaN at `missing` pixels (a count, or a fraction of the grid) drawn
    with `seed`; returns (Xn, Yn, flat indices of the missing pixels)."""
    d, T = X.shape[0], Y.shape[-1]
    n = Y[..., 0].size
    m = missing if isinstance(missing, int) else int(round(missing * n))
    miss = np.random.default_rng(seed).choice(n, m, replace=False)
    Xn, Yn = X.copy().reshape(d, -1), Y.copy().reshape(-1, T)
    Xn[:, miss] = np.nan
    Yn[miss] = np.nan
    return Xn.reshape(X.shape), Yn.reshape(Y.shape), miss


def pair(Xn, Yn, kernel, independent, lengthscale, isotropic=False, **kw):
    """(border, dense) reconstructors of the same incomplete grid."""
    import gpim_amd
    from gpim_amd import gprutils
    S = gprutils.border_blocks_multi(Xn, Yn)         # (seeded masks at these sizes leave no row or column empty)
    assert len(S["miss"]) == np.isnan(Yn[..., 0]).sum() > 0
    rb = gpim_amd.vreconstructor(Xn, Yn, kernel=kernel, lengthscale=lengthscale, independent=independent, verbose=0,
                                 isotropic=isotropic, solver="border", **kw)
    rd = gpim_amd.vreconstructor(Xn, Yn, kernel=kernel, lengthscale=lengthscale, independent=independent, verbose=0,
                                 isotropic=isotropic, solver="dense", **kw)
    assert rb.solver == "border" and rd.solver == "dense"
    assert torch.equal(rb.X, rd.X) and torch.equal(rb.y, rd.y) and rb.X.shape[0] == S["n_obs"]
    return rb, rd


def test_solver_choice():
    import gpim_amd
    Z = eels_twin(size=128, T=3, seed=1)
    X = gpim_amd.utils.get_full_grid(Z[..., 0])
    for frac in (0.05, 0.30):                        # flop ratios 0.09 and 0.74
        Xn, Zn, miss = knock_out(X, Z, frac, seed=7)
        rec = gpim_amd.vreconstructor(Xn, Zn, kernel="Matern52", lengthscale=[0.5, 2.5], verbose=0)
        assert rec.solver == "border", frac
        assert rec.X.shape == (128 * 128 - len(miss), 2)
    Rs, _ = spiral_image(size=128)                   # 74 % missing: the border is larger than what is left
    hole = np.isnan(Rs)
    Zs, Xs = Z.copy(), X.copy()
    Zs[hole] = np.nan
    Xs[:, hole] = np.nan
    assert hole.mean() > 0.7
    assert gpim_amd.vreconstructor(Xs, Zs, kernel="Matern52", verbose=0).solver == "dense"
    Zr, Xr = Z.copy(), X.copy()                      # an image row without any observation: the grid cannot be completed
    Zr[40] = np.nan
    Xr[:, 40] = np.nan
    assert gpim_amd.vreconstructor(Xr, Zr, kernel="Matern52", verbose=0).solver == "dense"
    with pytest.raises(NotImplementedError):
        gpim_amd.vreconstructor(Xr, Zr, kernel="Matern52", verbose=0, solver="border")
    pts, vals = X.reshape(2, -1).T[:200].copy(), Z.reshape(-1, 3)[:200].copy()
    pts[5] = np.nan                                  # scattered points with a NaN row: no grid to complete
    vals[5] = np.nan
    Xc, Yc = scattered(pts, vals)
    with pytest.raises(NotImplementedError):
        gpim_amd.vreconstructor(Xc, Yc, kernel="Matern52", verbose=0, solver="border")
    with pytest.raises(NotImplementedError):         # a complete grid has no border
        gpim_amd.vreconstructor(X, Z, kernel="Matern52", verbose=0, solver="border")
    with pytest.raises(NotImplementedError):
        gpim_amd.vreconstructor(Xn, Zn, kernel="Matern52", verbose=0, solver="reflection")
    assert gpim_amd.vreconstructor(X, Z, kernel="Matern52", verbose=0, solver="dense").solver == "dense"


LOSS_CASES = [  # kernel, shape, T, missing, independent, isotropic, lengthscale
    ("RBF", (32, 32), 3, 1, False, False, [0.5, 3.0]),
    ("Matern52", (32, 32), 6, 0.05, True, True, None),
    ("Matern52", (31, 32), 1, 0.10, False, False, [[0.5, 0.4], [2.5, 3.0]]),
    ("RBF", (31, 32), 16, 0.05, True, False, None),
    ("Matern52", (33, 33), 3, 0.30, False, True, [0.5, 2.5]),
    ("RBF", (33, 33), 6, 0.10, True, False, [0.5, 2.5]),
    ("Matern52", (16, 16, 15), 3, 0.05, False, False, [0.5, 2.5]),
    ("RBF", (16, 16, 15), 1, 0.30, True, True, None),
    ("RBF", (64, 64), 6, 0.30, False, False, [0.5, 3.0]),
    ("Matern52", (64, 64), 16, 0.05, True, False, None),
    ("Matern52", (12, 12), 3, 1, False, False, [0.5, 2.5]),        # far below the floor: one padded tile per block
]


@pytest.mark.parametrize("kernel,shape,T,missing,independent,isotropic,lengthscale", LOSS_CASES)
def test_loss_grad_against_dense_engine(kernel, shape, T, missing, independent, isotropic, lengthscale):
    X, Y = grid_stack(shape, T, seed=T + len(shape))
    Xn, Yn, _ = knock_out(X, Y, missing, seed=3 * T + shape[0])
    rb, rd = pair(Xn, Yn, kernel, independent, lengthscale, isotropic)
    n_ls = 1 if isotropic else len(shape)
    for k in range(2):
        u = V.random_u(T, n_ls, independent, seed=11 * k + T)
        l0, g0 = rd.nll_grad(u)
        l1, g1 = rb.nll_grad(u)
        el, eg = abs(l1 - l0) / abs(l0), np.abs(g1 - g0).max() / np.abs(g0).max()
        print("vgp border", kernel, shape, T, missing, "loss dev %.2e grad dev %.2e" % (el, eg))
        assert el <= 1e-9, (l1, l0)
        assert eg <= 1e-9, eg


@pytest.mark.parametrize("independent", [False, True])
def test_training_history_against_dense_engine(independent):
    X, Y = grid_stack((33, 30), 3, seed=4)
    Xn, Yn, _ = knock_out(X, Y, 0.05, seed=9)
    rb, rd = pair(Xn, Yn, "Matern52", independent, [0.5, 2.5], learning_rate=0.05, iterations=50)
    assert np.array_equal(rb._u.cpu().numpy(), rd._u.cpu().numpy())
    rb.train()
    rd.train()
    hb, hd = np.array(rb.hyperparams["lengthscale"]), np.array(rd.hyperparams["lengthscale"])
    assert hb.shape == hd.shape == (50, 2)
    lb, ld = np.array(rb.loss_all), np.array(rd.loss_all)
    rel = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max()
    print("vgp border training: lengthscale %.2e loss %.2e task_covar %.2e noise %.2e mean %.2e"
          % (rel(hb, hd), rel(lb, ld), rel(rb.task_covar, rd.task_covar), rel(rb.noise, rd.noise),
             rel(rb.mean_constants, rd.mean_constants)))
    assert np.allclose(hb, hd, rtol=1e-6, atol=0)
    assert np.allclose(lb, ld, rtol=1e-6, atol=0)
    assert np.allclose(rb.task_covar, rd.task_covar, rtol=1e-6, atol=0)
    assert np.allclose(rb.noise, rd.noise, rtol=1e-6, atol=0)
    assert np.allclose(rb.mean_constants, rd.mean_constants, rtol=1e-6, atol=0)


@pytest.mark.parametrize("kernel,shape,independent,missing", [("Matern52", (24, 19), False, 0.10), ("RBF", (17, 20), True, 0.05),
                                                              ("Matern52", (12, 10, 9), True, 0.10)])
def test_prediction_against_dense_engine(kernel, shape, independent, missing):
    check_prediction(kernel, shape, independent, missing, lambda rec, X: rec.predict(X))


@pytest.mark.parametrize("kernel,shape,independent,missing", [("Matern52", (24, 19), False, 0.10), ("RBF", (17, 20), True, 0.05)])
def test_prediction_in_chunks_against_dense_engine(monkeypatch, kernel, shape, independent, missing):
    """The bordered blocks' prediction in chunks of 128 test columns (the border's R = sum_b Y_b^T K*_b per chunk): the
    training grids of 456 and 340 points take four and three chunks with a ragged last one."""
    check_prediction(kernel, shape, independent, missing, chunked_predict(monkeypatch))


def check_prediction(kernel, shape, independent, missing, predict):
    import gpim_amd
    T = 4
    X, Y = grid_stack(shape, T, seed=21)
    Xn, Yn, miss = knock_out(X, Y, missing, seed=13)
    rb, rd = pair(Xn, Yn, kernel, independent, [0.3, 3.0])
    u = V.random_u(T, len(shape), independent, seed=5)
    rb._u.copy_(torch.as_tensor(u))
    rd._u.copy_(torch.as_tensor(u))
    scale = np.abs(Y).max()
    m1, s1 = predict(rb, X)                              # the training grid, missing pixels included
    m0, s0 = rd.predict(X)
    assert m1.shape == s1.shape == X.shape[1:] + (T,)
    print("vgp border predict grid: mean %.2e sd %.2e" % (np.abs(m1 - m0).max() / scale, np.abs(s1 - s0).max() / scale))
    assert np.abs(m1 - m0).max() <= 1e-9 * scale and np.abs(s1 - s0).max() <= 1e-9 * scale
    sd_miss = s1.reshape(-1, T)[miss]
    assert np.isfinite(sd_miss).all() and (sd_miss > 0).all()
    Xd = gpim_amd.utils.get_full_grid(Y[..., 0], dense_x=0.5)
    m1, s1 = predict(rb, Xd)
    m0, s0 = rd.predict(Xd)
    assert m1.shape == s1.shape == Xd.shape[1:] + (T,)
    assert np.abs(m1 - m0).max() <= 1e-9 * scale and np.abs(s1 - s0).max() <= 1e-9 * scale
    rng = np.random.default_rng(3)
    Xs = rng.uniform(-1.5, max(shape) + 1.5, size=(len(shape), 37))
    Xs[:, 5] = np.nan
    Xs[1, 20] = np.nan
    m1, s1 = predict(rb, Xs)
    m0, s0 = rd.predict(Xs)
    nan = np.isnan(Xs).any(0)
    assert np.isnan(m1[nan]).all() and np.isnan(s1[nan]).all()
    assert np.abs(m1[~nan] - m0[~nan]).max() <= 1e-9 * scale
    assert np.abs(s1[~nan] - s0[~nan]).max() <= 1e-9 * scale


def test_runs_are_bitwise_identical():
    import gpim_amd
    X, Y = grid_stack((31, 30), 5, seed=2)
    Xn, Yn, _ = knock_out(X, Y, 0.10, seed=6)
    hs = []
    for _ in range(2):
        rec = gpim_amd.vreconstructor(Xn, Yn, kernel="Matern52", lengthscale=[0.5, 2.5], learning_rate=0.05, iterations=30,
                                      verbose=0, solver="border")
        assert rec.solver == "border"
        rec.train()
        mean, sd = rec.predict(X)
        hs.append((np.array(rec.hyperparams["lengthscale"]), np.array(rec.loss_all), rec._u.cpu().numpy(), mean, sd))
    assert len(hs[0][0]) == 30 and np.isfinite(hs[0][3]).all() and np.isfinite(hs[0][4]).all()
    for a, b in zip(*hs):
        assert np.array_equal(a, b)


def _nll_grad_raw(rec, S, wts_d, border=None):
    """gpimhip_vgp_nll_grad on rec's handle in reflection mode with the blocks S, optionally after gpimhip_set_border
    (M, q, coef); returns (rc, loss, grad)."""
    from gpim_amd import _lib
    lib, h = rec._handle.lib, rec._handle.h
    u = rec._u.clone()
    out = torch.zeros(u.numel() + 1, dtype=torch.float64, device=u.device)
    _lib.check(lib.gpimhip_set_reflection(h, S["mask"], rec._blocks.twoc, _lib.ptr(wts_d), S["n_total"], 0))
    try:
        if border is not None:
            M, q_d, coef_d = border
            _lib.check(lib.gpimhip_set_border(h, M, None if q_d is None else ctypes.c_void_p(q_d.data_ptr()), _lib.ptr(coef_d)))
        rc = lib.gpimhip_vgp_nll_grad(h, ctypes.byref(rec._mstruct), ctypes.byref(rec._vstruct), _lib.ptr(rec._Xd),
                                      _lib.ptr(rec._Yd), rec._Xd.shape[0], _lib.ptr(u), _lib.ptr(out), _lib.ptr(out[1:]))
    finally:
        _lib.check(lib.gpimhip_set_reflection(h, 0, None, None, 0, 0))
    o = out.cpu().numpy()
    return rc, o[0], o[1:]


def test_border_on_sharded_handle_is_rejected():
    from gpim_amd import _lib
    X, Y = grid_stack((16, 16), 2, seed=1)
    Xn, Yn, _ = knock_out(X, Y, 0.05, seed=2)
    rb, _ = pair(Xn, Yn, "RBF", False, None)
    lib, h = rb._handle.lib, rb._handle.h
    S = rb._refl
    u = rb._u.clone()
    out = torch.empty(u.numel() + 1, dtype=torch.float64, device=u.device)
    _lib.check(lib.gpimhip_set_reflection(h, S["mask"], rb._blocks.twoc, _lib.ptr(rb._blocks.wts), S["n_total"], 0))
    try:
        _lib.check(lib.gpimhip_set_border(h, len(S["miss"]), ctypes.c_void_p(rb._blocks.q.data_ptr()), _lib.ptr(rb._blocks.coef)))
        _lib.check(lib.gpimhip_set_reflection_shard(h, 0, 2, S["B"], 0))
        rc = lib.gpimhip_vgp_nll_grad(h, ctypes.byref(rb._mstruct), ctypes.byref(rb._vstruct), _lib.ptr(rb._Xd),
                                      _lib.ptr(rb._Yd), rb._Xd.shape[0], _lib.ptr(u), _lib.ptr(out), _lib.ptr(out[1:]))
        assert rc == _lib.E_BADARG
    finally:
        _lib.check(lib.gpimhip_set_reflection(h, 0, None, None, 0, 0))
    l0, _ = rb.nll_grad()
    assert np.isfinite(l0)


def test_empty_border_gives_the_bits_of_the_complete_grid():
    import gpim_amd
    X, Y = grid_stack((15, 14), 3, seed=8)
    rr = gpim_amd.vreconstructor(X, Y, kernel="Matern52", lengthscale=[0.5, 2.5], verbose=0)
    assert rr.solver == "reflection"
    rc0, l0, g0 = _nll_grad_raw(rr, rr._refl, rr._blocks.wts)
    rc1, l1, g1 = _nll_grad_raw(rr, rr._refl, rr._blocks.wts, border=(0, None, None))
    assert rc0 == 0 and rc1 == 0
    assert np.array_equal(l0, l1) and np.array_equal(g0, g1)
    # ... also after the handle has carried a real border
    Xn, Yn, _ = knock_out(X, Y, 0.05, seed=2)
    rb, _ = pair(Xn, Yn, "Matern52", False, [0.5, 2.5])
    assert np.isfinite(rb.nll_grad()[0])
    rb._Yd = rr._Yd.to(rb._dev)          # (the completed grid's domain and weights are rr's own)
    rc2, l2, g2 = _nll_grad_raw(rb, rr._refl, rr._blocks.wts.to(rb._dev), border=(0, None, None))
    assert rc2 == 0 and np.array_equal(l0, l2) and np.array_equal(g0, g2)


# ---------------------------------------------------------------------------------------------------------------------
# full size
# ---------------------------------------------------------------------------------------------------------------------
def border_bytes(n_grid, M, T, r=2):
    """section 12's 3 T B np (np + 16) doubles plus 2 T B np mp for C and Y and 3 T mp (mp + 16) for
    the borders' own workspace (np, mp: N_q and M padded to 128; the 16: the padded leading dimension from 1024 on)."""
    B = 1 << r
    np_, mp = -(-(n_grid // B) // 128) * 128, -(-M // 128) * 128
    ld = lambda n: n + (16 if n >= 1024 else 0)
    return 8 * (3 * T * B * np_ * ld(np_) + 2 * T * B * np_ * mp + 3 * T * mp * ld(mp))


def test_128x128x3_against_dense_engine():
    Z = eels_twin(size=128, T=3, seed=3)
    X = np.array(np.meshgrid(np.arange(128.0), np.arange(128.0), indexing="ij"))
    Xn, Zn, miss = knock_out(X, Z, 0.05, seed=5)
    rb, rd = pair(Xn, Zn, "Matern52", False, [0.5, 2.5])
    u = rb._u.cpu().numpy()
    l0, g0 = rd.nll_grad(u)
    l1, g1 = rb.nll_grad(u)
    el, eg = abs(l1 - l0) / abs(l0), np.abs(g1 - g0).max() / np.abs(g0).max()
    ws = rb._handle.lib.gpimhip_workspace_bytes(rb._handle.h)
    print("vgp border 128x128x3: loss dev %.2e grad dev %.2e workspace %d (formula %d)" % (el, eg, ws, border_bytes(128 * 128, len(miss), 3)))
    assert el <= 1e-9, (l1, l0)
    assert eg <= 1e-9, eg
    assert 0 < ws <= 1.10 * border_bytes(128 * 128, len(miss), 3), ws


def test_256x256x6_two_percent_five_iterations():
    import gpim_amd
    Z = eels_twin(size=256, T=6, seed=4)
    X = gpim_amd.utils.get_full_grid(Z[..., 0])
    Xn, Zn, miss = knock_out(X, Z, 0.02, seed=5)
    rec = gpim_amd.vreconstructor(Xn, Zn, kernel="Matern52", lengthscale=[0.5, 2.5], learning_rate=0.05, iterations=5,
                                  verbose=0, solver="border")
    assert rec.solver == "border"
    rec.train()
    hist = np.array(rec.hyperparams["lengthscale"])
    assert hist.shape == (5, 2) and np.isfinite(hist).all() and np.isfinite(rec.loss_all).all()
    assert np.all((hist > 0.5) & (hist < 2.5))
    assert np.all(np.diff(rec.loss_all) < 0), rec.loss_all
    ws = rec._handle.lib.gpimhip_workspace_bytes(rec._handle.h)
    print("vgp border 256x256x6: workspace %d (formula %d) loss %s" % (ws, border_bytes(256 * 256, len(miss), 6), rec.loss_all))
    assert 0 < ws <= 1.10 * border_bytes(256 * 256, len(miss), 6), ws
