"""vreconstructor's reflection solver (complete grids) on the MI355X against the dense engine on the
same data and parameters.  The dense engine is reached by passing the same points in the scattered layout of
test_gpu_vgp.scattered, whose (d, N, 1) X is not a product grid."""
import ctypes

import numpy as np
import pytest
import torch

import vgp_oracle as V
from test_gpu_vgp import eels_twin, scattered

pytestmark = pytest.mark.gpu


def grid_stack(shape, T, seed, spacing=None):
    """get_full_grid-style coordinates (d, *shape) and a smooth (*shape, T) stack of T correlated outputs."""
    axes = [np.arange(n, dtype=np.float64) * (1.0 if spacing is None else spacing[k]) for k, n in enumerate(shape)]
    X = np.array(np.meshgrid(*axes, indexing="ij"))
    rng = np.random.default_rng(seed)
    pts = X.reshape(X.shape[0], -1).T
    base = np.stack([np.sin(pts @ rng.normal(size=pts.shape[1]) * 0.4 + rng.uniform(0, 6)) for _ in range(3)], 1)
    Y = base @ rng.normal(size=(3, T)) + 0.1 * rng.normal(size=(pts.shape[0], T)) + rng.normal(size=T)
    return X, Y.reshape(tuple(shape) + (T,))


def pair(X, Y, kernel, independent, lengthscale, isotropic=False, **kw):
    """(reflection, dense) reconstructors of the same data."""
    import gpim_amd
    d, T = X.shape[0], Y.shape[-1]
    rr = gpim_amd.vreconstructor(X, Y, kernel=kernel, lengthscale=lengthscale, independent=independent, verbose=0,
                                 isotropic=isotropic, **kw)
    Xs, Ys = scattered(X.reshape(d, -1).T, Y.reshape(-1, T))
    rd = gpim_amd.vreconstructor(Xs, Ys, kernel=kernel, lengthscale=lengthscale, independent=independent, verbose=0,
                                 isotropic=isotropic, **kw)
    assert rr.solver == "reflection" and rd.solver == "dense"
    assert torch.equal(rr.X, rd.X) and torch.equal(rr.y, rd.y)
    return rr, rd


def test_solver_choice():
    import gpim_amd
    Z = eels_twin(size=12, T=3)
    X = gpim_amd.utils.get_full_grid(Z[..., 0])
    rec = gpim_amd.vreconstructor(X, Z, kernel="Matern52", lengthscale=[0.5, 2.5], verbose=0)
    assert rec.solver == "reflection"
    assert rec.X.shape == (144, 2) and rec.y.shape == (144, 3)
    Xs, Ys = scattered(rec.X.numpy(), rec.y.numpy())
    assert gpim_amd.vreconstructor(Xs, Ys, kernel="Matern52", verbose=0).solver == "dense"
    Zn = Z.copy()
    Zn[3, 4, 1] = np.nan                      # a NaN row: the observed points are no complete grid
    Xn = X.copy()
    Xn[:, 3, 4] = np.nan
    rn = gpim_amd.vreconstructor(Xn, Zn, kernel="Matern52", lengthscale=[0.5, 2.5], verbose=0)
    assert rn.solver == "dense" and rn.X.shape == (143, 2)
    Xa = X.copy()
    Xa[0] = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12.5])[:, None]   # axis 0 not symmetric, axis 1 still is
    assert gpim_amd.vreconstructor(Xa, Z, kernel="RBF", verbose=0).solver == "reflection"
    Xb = X.copy()
    Xb[1] = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12.5])[None, :]
    Xb[0] = Xa[0]
    assert gpim_amd.vreconstructor(Xb, Z, kernel="RBF", verbose=0).solver == "dense"       # no symmetric axis


LOSS_CASES = [  # kernel, shape, T, independent, isotropic, lengthscale
    ("RBF", (16, 16), 3, False, False, [0.5, 3.0]),
    ("Matern52", (16, 16), 6, True, True, None),
    ("RBF", (15, 12), 1, True, False, None),
    ("Matern52", (15, 12), 16, False, False, [[0.5, 0.4], [2.5, 3.0]]),
    ("Matern52", (9, 9), 3, False, True, [0.5, 2.5]),
    ("RBF", (9, 9), 6, True, False, [0.5, 2.5]),
    ("RBF", (40, 40), 6, False, False, [0.5, 3.0]),
    ("Matern52", (40, 40), 3, True, False, None),
    ("Matern52", (8, 6, 5), 3, False, False, [0.5, 2.5]),
    ("RBF", (8, 6, 5), 16, True, True, None),
]


@pytest.mark.parametrize("kernel,shape,T,independent,isotropic,lengthscale", LOSS_CASES)
def test_loss_grad_against_dense_engine(kernel, shape, T, independent, isotropic, lengthscale):
    X, Y = grid_stack(shape, T, seed=T + len(shape))
    rr, rd = pair(X, Y, kernel, independent, lengthscale, isotropic)
    n_ls = 1 if isotropic else len(shape)
    for k in range(2):
        u = V.random_u(T, n_ls, independent, seed=11 * k + T)
        l0, g0 = rd.nll_grad(u)
        l1, g1 = rr.nll_grad(u)
        assert abs(l1 - l0) <= 1e-10 * abs(l0), (l1, l0)
        assert np.abs(g1 - g0).max() <= 1e-10 * np.abs(g0).max(), np.abs(g1 - g0).max() / np.abs(g0).max()


@pytest.mark.parametrize("independent", [False, True])
def test_training_history_against_dense_engine(independent):
    X, Y = grid_stack((13, 10), 3, seed=4)
    rr, rd = pair(X, Y, "Matern52", independent, [0.5, 2.5], learning_rate=0.05, iterations=100)
    assert np.array_equal(rr._u.cpu().numpy(), rd._u.cpu().numpy())
    rr.train()
    rd.train()
    hr, hd = np.array(rr.hyperparams["lengthscale"]), np.array(rd.hyperparams["lengthscale"])
    assert hr.shape == hd.shape == (100, 2)
    assert np.abs(hr - hd).max() <= 1e-7 * np.abs(hd).max()
    assert np.abs(np.array(rr.loss_all) - np.array(rd.loss_all)).max() <= 1e-9 * np.abs(rd.loss_all).max()
    assert np.allclose(rr.task_covar, rd.task_covar, rtol=1e-7, atol=1e-9 * np.abs(rd.task_covar).max())
    assert np.allclose(rr.noise, rd.noise, rtol=1e-7)
    assert np.allclose(rr.mean_constants, rd.mean_constants, rtol=1e-7, atol=1e-9)
    assert np.allclose(rr.lengthscale, rd.lengthscale, rtol=1e-7)


@pytest.mark.parametrize("kernel,shape,independent", [("Matern52", (12, 9), False), ("RBF", (7, 10), True),
                                                      ("Matern52", (6, 5, 4), True)])
def test_prediction_against_dense_engine(kernel, shape, independent):
    check_prediction(kernel, shape, independent, lambda rec, X: rec.predict(X))


def chunked_predict(monkeypatch):
    """predict() of the model under test with GPIMHIP_PREDICT_CHUNK=128 (the dense reference of the same test runs without)."""
    def predict(rec, X):
        monkeypatch.setenv("GPIMHIP_PREDICT_CHUNK", "128")
        try:
            return rec.predict(X)
        finally:
            monkeypatch.delenv("GPIMHIP_PREDICT_CHUNK")
    return predict


@pytest.mark.parametrize("kernel,shape,independent", [("Matern52", (12, 9), False), ("RBF", (16, 16), True)])
def test_prediction_in_chunks_against_dense_engine(monkeypatch, kernel, shape, independent):
    """The blocks' prediction in chunks of 128 test columns: the x2 grids of 391 and 961 points take four and eight chunks
    with a ragged last one."""
    check_prediction(kernel, shape, independent, chunked_predict(monkeypatch))


def check_prediction(kernel, shape, independent, predict):
    import gpim_amd
    T = 4
    X, Y = grid_stack(shape, T, seed=21)
    rr, rd = pair(X, Y, kernel, independent, [0.3, 3.0])
    u = V.random_u(T, len(shape), independent, seed=5)
    rr._u.copy_(torch.as_tensor(u))
    rd._u.copy_(torch.as_tensor(u))
    scale = np.abs(Y).max()
    Xd = gpim_amd.utils.get_full_grid(Y[..., 0], dense_x=0.5)
    m1, s1 = predict(rr, Xd)
    m0, s0 = rd.predict(Xd)
    assert m1.shape == s1.shape == Xd.shape[1:] + (T,)
    assert np.abs(m1 - m0).max() <= 1e-9 * scale and np.abs(s1 - s0).max() <= 1e-9 * scale
    rng = np.random.default_rng(3)
    Xs = rng.uniform(-1.5, max(shape) + 1.5, size=(len(shape), 37))
    Xs[:, 5] = np.nan
    Xs[1, 20] = np.nan
    m1, s1 = predict(rr, Xs)
    m0, s0 = rd.predict(Xs)
    nan = np.isnan(Xs).any(0)
    assert np.isnan(m1[nan]).all() and np.isnan(s1[nan]).all()
    assert np.abs(m1[~nan] - m0[~nan]).max() <= 1e-9 * scale
    assert np.abs(s1[~nan] - s0[~nan]).max() <= 1e-9 * scale


def test_runs_are_bitwise_identical():
    import gpim_amd
    X, Y = grid_stack((15, 14), 5, seed=2)
    hs = []
    for _ in range(2):
        rec = gpim_amd.vreconstructor(X, Y, kernel="Matern52", lengthscale=[0.5, 2.5], learning_rate=0.05, iterations=30,
                                      verbose=0)
        assert rec.solver == "reflection"
        rec.train()
        mean, sd = rec.predict(X)
        hs.append((np.array(rec.hyperparams["lengthscale"]), np.array(rec.loss_all), rec._u.cpu().numpy(), mean, sd))
    for a, b in zip(*hs):
        assert np.array_equal(a, b)


def test_graph_replay_equals_eager_launches(monkeypatch):
    """solver='reflection': one captured iteration replayed (default) against the same launches enqueued iteration by
    iteration (GPIMHIP_NO_GRAPH=1) -- the same bits in the histories, the parameters and the posterior."""
    import gpim_amd
    X, Y = grid_stack((15, 14), 5, seed=2)
    hs = []
    for knob in (None, "1"):
        if knob:
            monkeypatch.setenv("GPIMHIP_NO_GRAPH", knob)
        else:
            monkeypatch.delenv("GPIMHIP_NO_GRAPH", raising=False)
        rec = gpim_amd.vreconstructor(X, Y, kernel="Matern52", lengthscale=[0.5, 2.5], learning_rate=0.05, iterations=30,
                                      verbose=0)
        assert rec.solver == "reflection"
        rec.train()
        mean, sd = rec.predict(X)
        hs.append((np.array(rec.hyperparams["lengthscale"]), np.array(rec.loss_all), rec._u.cpu().numpy(), mean, sd))
    assert all(np.isfinite(a).all() for a in hs[0])
    for a, b in zip(*hs):
        assert np.array_equal(a, b)


def test_reflection_mode_rejects_sharded_handle():
    from gpim_amd import _lib
    X, Y = grid_stack((8, 8), 2, seed=1)
    rr, _ = pair(X, Y, "RBF", False, None)
    lib, h = rr._handle.lib, rr._handle.h
    S = rr._refl
    u = rr._u.clone()
    out = torch.empty(u.numel() + 1, dtype=torch.float64, device=u.device)
    _lib.check(lib.gpimhip_set_reflection(h, S["mask"], rr._blocks.twoc, None, S["n_total"], 0))
    try:
        _lib.check(lib.gpimhip_set_reflection_shard(h, 0, 2, S["B"], 0))
        rc = lib.gpimhip_vgp_nll_grad(h, ctypes.byref(rr._mstruct), ctypes.byref(rr._vstruct), _lib.ptr(rr._Xd),
                                      _lib.ptr(rr._Yd), rr._Xd.shape[0], _lib.ptr(u), _lib.ptr(out), _lib.ptr(out[1:]))
        assert rc == _lib.E_BADARG
    finally:
        _lib.check(lib.gpimhip_set_reflection(h, 0, None, None, 0, 0))
    l0, _ = rr.nll_grad()
    assert np.isfinite(l0)


# ---------------------------------------------------------------------------------------------------------------------
# full size
# ---------------------------------------------------------------------------------------------------------------------
def test_128x128x3_against_dense_engine():
    Z = eels_twin(size=128, T=3, seed=3)
    X = np.array(np.meshgrid(np.arange(128.0), np.arange(128.0), indexing="ij"))
    rr, rd = pair(X, Z, "Matern52", False, [0.5, 2.5])
    u = rr._u.cpu().numpy()
    l0, g0 = rd.nll_grad(u)
    l1, g1 = rr.nll_grad(u)
    assert abs(l1 - l0) <= 1e-10 * abs(l0), (l1, l0)
    assert np.abs(g1 - g0).max() <= 1e-9 * np.abs(g0).max(), np.abs(g1 - g0).max() / np.abs(g0).max()


def test_256x256x6_five_iterations():
    import gpim_amd
    Z = eels_twin(size=256, T=6, seed=4)
    X = gpim_amd.utils.get_full_grid(Z[..., 0])
    rec = gpim_amd.vreconstructor(X, Z, kernel="Matern52", lengthscale=[0.5, 2.5], learning_rate=0.05, iterations=5,
                                  verbose=0)
    assert rec.solver == "reflection"
    rec.train()
    hist = np.array(rec.hyperparams["lengthscale"])
    assert hist.shape == (5, 2) and np.isfinite(hist).all() and np.isfinite(rec.loss_all).all()
    assert np.all((hist > 0.5) & (hist < 2.5))
    ws = rec._handle.lib.gpimhip_workspace_bytes(rec._handle.h)
    assert 0 < ws < 170e9, ws
