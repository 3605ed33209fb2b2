"""The exact multi-output GP (gpim_amd.vreconstructor / gpim.gpreg.vgpr.vreconstructor) on the MI355X against the dense
restatement of tests/vgp_oracle.py (N T x N T covariance, torch autograd and Adam on the CPU)."""
import ctypes

import numpy as np
import pytest
import torch

import vgp_oracle as V

pytestmark = pytest.mark.gpu


def scattered(X, Y):
    """(N, d) points, (N, T) outputs -> the reference's (c, *dims) / (*dims, T) arrays with dims = (N, 1, ...)."""
    N, d = X.shape
    dims = (N,) + (1,) * (d - 1)
    return np.ascontiguousarray(X.T).reshape((d,) + dims), Y.reshape(dims + (Y.shape[1],))


def make(X, Y, kernel, independent, bounds, isotropic, **kw):
    import gpim_amd
    Xg, Yg = scattered(X, Y)
    lengthscale = None if bounds is None else [bounds[0], bounds[1]]
    return gpim_amd.vreconstructor(Xg, Yg, kernel=kernel, lengthscale=lengthscale, independent=independent,
                                   verbose=0, isotropic=isotropic, **kw)


CASES = [  # kernel, d, isotropic, independent, T, N, bounds
    ("RBF", 2, False, False, 3, 100, ([0.5, 0.3], [2.5, 4.0])),
    ("Matern52", 2, True, True, 6, 100, (0.5, 2.5)),
    ("Matern52", 3, False, False, 1, 300, (0.5, 3.0)),
    ("RBF", 3, True, True, 3, 300, None),
    ("RBF", 2, False, True, 1, 1000, (0.2, 3.0)),
    ("Matern52", 2, False, False, 3, 1000, (0.5, 2.5)),
    ("RBF", 3, False, False, 6, 300, ([0.5, 0.5, 0.5], [3.0, 3.0, 3.0])),
    ("Matern52", 3, True, False, 6, 130, None),
]


@pytest.mark.parametrize("kernel,d,iso,indep,T,N,bounds", CASES)
def test_loss_grad_against_dense(kernel, d, iso, indep, T, N, bounds):
    X, Y = V.random_data(N, T, d, seed=N + T)
    rec = make(X, Y, kernel, indep, bounds, iso)
    dense = V.Dense(X, Y, kernel, indep, bounds, iso)
    n_ls = 1 if iso else d
    for k in range(2):
        u = V.random_u(T, n_ls, indep, seed=100 * k + T)
        l0, g0 = dense.loss_grad(u)
        l1, g1 = rec.nll_grad(u)
        assert abs(l1 - l0) <= 1e-10 * abs(l0), (l1, l0)
        assert np.abs(g1 - g0).max() <= 1e-10 * np.abs(g0).max(), np.abs(g1 - g0).max() / np.abs(g0).max()


@pytest.mark.parametrize("independent", [False, True])
def test_training_history_against_dense(independent):
    X, Y = V.random_data(150, 3, 2, seed=11)
    bounds = (0.5, 2.5)
    rec = make(X, Y, "Matern52", independent, bounds, False, learning_rate=0.05, iterations=100)
    dense = V.Dense(X, Y, "Matern52", independent, bounds)
    u0 = rec._u.cpu().numpy()
    assert np.array_equal(u0, V.initial_u(3, 2, independent))
    hist, losses, u_end = dense.fit(u0, 0.05, 100)
    rec.train()
    got = np.array(rec.hyperparams["lengthscale"])
    assert got.shape == (100, 2)
    assert np.abs(got - hist).max() <= 1e-7 * np.abs(hist).max()
    assert np.abs(np.array(rec.loss_all) - losses).max() <= 1e-9 * np.abs(losses).max()
    mu, B, s, ls = (t.numpy() for t in dense.params(u_end))
    assert np.allclose(rec.task_covar, B, rtol=1e-7, atol=1e-9 * np.abs(B).max())
    assert np.allclose(rec.noise, s, rtol=1e-7)
    assert np.allclose(rec.mean_constants, mu, rtol=1e-7, atol=1e-9)
    assert np.allclose(rec.lengthscale, ls, rtol=1e-7)


@pytest.mark.parametrize("independent,kernel,N", [(False, "Matern52", 200), (True, "RBF", 90), (False, "RBF", 700)])
def test_prediction_against_dense(independent, kernel, N):
    T = 4
    X, Y = V.random_data(N, T, 2, seed=21, scale=3.0)
    rec = make(X, Y, kernel, independent, (0.3, 3.0), False)
    u = V.random_u(T, 2, independent, seed=5)
    rec._u.copy_(torch.as_tensor(u))
    g = np.stack(np.meshgrid(np.linspace(-0.5, 8.5, 13), np.linspace(-0.5, 8.5, 11), indexing="ij"))   # (2, 13, 11)
    g[:, 3, 4] = np.nan
    g[:, 7, :] = np.nan
    mean, sd = rec.predict(g)
    assert mean.shape == sd.shape == (13, 11, T)
    Xs = g.reshape(2, -1).T
    mo, vo = V.Dense(X, Y, kernel, independent, (0.3, 3.0)).predict(u, Xs)
    mo, so = mo.reshape(13, 11, T), np.sqrt(vo).reshape(13, 11, T)
    nan = np.isnan(Xs).any(1).reshape(13, 11)
    assert np.isnan(mean[nan]).all() and np.isnan(sd[nan]).all()
    scale = np.abs(Y).max()
    assert np.abs(mean[~nan] - mo[~nan]).max() <= 1e-9 * scale
    assert np.abs(sd[~nan] - so[~nan]).max() <= 1e-9 * scale


def test_correlated_without_factor_equals_independent():
    """F = 0 turns the MultitaskKernel into B = diag(softplus(r_v)): the independent model with r_o = r_v."""
    T, N = 3, 160
    X, Y = V.random_data(N, T, 2, seed=8)
    rc = make(X, Y, "RBF", False, (0.5, 2.5), False)
    ri = make(X, Y, "RBF", True, (0.5, 2.5), False)
    ui = V.random_u(T, 2, True, seed=4)
    uc = np.concatenate([ui[:T], np.zeros(T), ui[T:]])         # [mu | F = 0 | r_v = r_o | r_l | r_a | r_g]
    lc, gc = rc.nll_grad(uc)
    li, gi = ri.nll_grad(ui)
    assert abs(lc - li) <= 1e-13 * abs(li)
    gref = np.concatenate([gi[:T], np.zeros(T), gi[T:]])
    assert np.abs(gc - gref).max() <= 1e-13 * np.abs(gi).max()
    rc._u.copy_(torch.as_tensor(uc))
    ri._u.copy_(torch.as_tensor(ui))
    Xs = np.random.default_rng(0).uniform(0, 8, size=(2, 50))
    mc, sc = rc.predict(Xs)
    mi, si = ri.predict(Xs)
    assert np.abs(mc - mi).max() <= 1e-13 * np.abs(mi).max() and np.abs(sc - si).max() <= 1e-13 * np.abs(si).max()


def test_runs_are_bitwise_identical():
    X, Y = V.random_data(260, 5, 2, seed=2)
    hs = []
    for _ in range(2):
        rec = make(X, Y, "Matern52", False, (0.5, 2.5), False, learning_rate=0.05, iterations=30)
        rec.train()
        hs.append((np.array(rec.hyperparams["lengthscale"]), np.array(rec.loss_all), rec._u.cpu().numpy()))
    for a, b in zip(*hs):
        assert np.array_equal(a, b)


def test_graph_replay_equals_eager_launches(monkeypatch):
    """One captured iteration replayed (default; N = 260 is far below the large-N regime, 30 iterations >= 8) against the same
    launches enqueued iteration by iteration (GPIMHIP_NO_GRAPH=1): the same bits in the histories, the parameters and the
    posterior (tests/test_gpu_regimes.py has the exact GP's case)."""
    X, Y = V.random_data(260, 5, 2, seed=2)
    Xs = np.random.default_rng(0).uniform(0, 8, size=(2, 50))
    hs = []
    for knob in (None, "1"):
        if knob:
            monkeypatch.setenv("GPIMHIP_NO_GRAPH", knob)
        else:
            monkeypatch.delenv("GPIMHIP_NO_GRAPH", raising=False)
        rec = make(X, Y, "Matern52", False, (0.5, 2.5), False, learning_rate=0.05, iterations=30)
        assert rec.solver == "dense"
        rec.train()
        mean, sd = rec.predict(Xs)
        hs.append((np.array(rec.hyperparams["lengthscale"]), np.array(rec.loss_all), rec._u.cpu().numpy(), mean, sd))
    assert all(np.isfinite(a).all() for a in hs[0])
    for a, b in zip(*hs):
        assert np.array_equal(a, b)


def test_invalid_arguments():
    import gpim_amd
    from gpim_amd import _lib
    X, Y = V.random_data(50, 2, 2, seed=1)
    with pytest.raises(NotImplementedError):
        make(X, Y, "Spectral", False, None, False)
    with pytest.raises(NotImplementedError):
        make(X, Y, "RBF", False, None, False, precision="single")
    rec = make(X, Y, "RBF", False, None, False)
    u = torch.zeros(64, dtype=torch.float64, device="cuda")
    out = torch.empty(64, dtype=torch.float64, device="cuda")
    lib, h = rec._handle.lib, rec._handle.h
    m = _lib.ModelStruct.from_buffer_copy(rec._mstruct)
    m.kernel = _lib.KERNEL_IDS["RationalQuadratic"]
    rc = lib.gpimhip_vgp_nll_grad(h, ctypes.byref(m), ctypes.byref(rec._vstruct), _lib.ptr(rec._Xd), _lib.ptr(rec._Yd),
                                  50, _lib.ptr(u), _lib.ptr(out), _lib.ptr(out[1:]))
    assert rc == _lib.E_BADARG
    vg = _lib.VgpStruct(17, 1, 0, 1)
    rc = lib.gpimhip_vgp_nll_grad(h, ctypes.byref(rec._mstruct), ctypes.byref(vg), _lib.ptr(rec._Xd), _lib.ptr(rec._Yd),
                                  50, _lib.ptr(u), _lib.ptr(out), _lib.ptr(out[1:]))
    assert rc == _lib.E_BADARG
    assert gpim_amd.vreconstructor is not None


# ---------------------------------------------------------------------------------------------------------------------
# full size: a twin of the reference notebook's EELS problem (GP_EELS.ipynb cell 19: 48 x 48 image, 6 NMF components)
# ---------------------------------------------------------------------------------------------------------------------
def eels_twin(size=48, T=6, seed=0):
    """A smooth synthetic 48 x 48 x 6 stack (the measured eels.npy is not part of the repository)."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
    Z = np.empty((size, size, T))
    for t in range(T):
        cx, cy = rng.uniform(8, 40, 2)
        w = rng.uniform(5, 12)
        Z[..., t] = (np.exp(-((i - cx) ** 2 + (j - cy) ** 2) / (2 * w * w)) + 0.3 * np.sin(i / rng.uniform(4, 9))
                     * np.cos(j / rng.uniform(4, 9)) + 0.02 * rng.normal(size=(size, size)))
    return Z


def test_eels_twin_full_size():
    import gpim_amd
    Z = eels_twin()
    X = gpim_amd.utils.get_full_grid(Z[..., 0])
    rec = gpim_amd.vreconstructor(X, Z, kernel="Matern52", lengthscale=[0.5, 2.5], learning_rate=0.05, iterations=200,
                                  verbose=0)
    Xn, Yn = rec.X.numpy(), rec.y.numpy()
    assert Xn.shape == (2304, 2) and Yn.shape == (2304, 6)
    u0 = rec._u.cpu().numpy()
    rng = np.random.default_rng(1)
    for u in (u0, u0 + 0.3 * rng.normal(size=u0.size), u0 + 0.6 * rng.normal(size=u0.size)):
        l0, g0 = V.reduction_loss_grad(u, Xn, Yn, "Matern52", False, (0.5, 2.5))
        l1, g1 = rec.nll_grad(u)
        assert abs(l1 - l0) <= 1e-10 * abs(l0)
        assert np.abs(g1 - g0).max() <= 1e-10 * np.abs(g0).max()
    rec.train()
    hist = np.array(rec.hyperparams["lengthscale"])
    assert hist.shape == (200, 2) and np.isfinite(hist).all() and np.isfinite(rec.loss_all).all()
    assert np.all((hist > 0.5) & (hist < 2.5))
    Xd = gpim_amd.utils.get_full_grid(Z[..., 0], dense_x=0.5)
    mean, sd = rec.predict(Xd)
    assert mean.shape == sd.shape == Xd.shape[1:] + (6,)
    assert np.isfinite(mean).all() and np.isfinite(sd).all() and (sd > 0).all()
