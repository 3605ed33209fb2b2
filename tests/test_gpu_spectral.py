"""The spectral-mixture kernel of skreconstructor(kernel='Spectral') on the MI355X (include/gpimhip.h: gpimhip_sm_*) against
the dense float64 restatement of tests/sm_oracle.py."""
import ctypes

import numpy as np
import pytest
import torch

import sm_oracle as S

pytestmark = pytest.mark.gpu


def scattered(X, y):
    """(N, d) points, (N,) values -> the reference's (c, *dims) / (*dims) arrays with dims = (N, 1, ...)."""
    N, d = X.shape
    dims = (N,) + (1,) * (d - 1)
    return np.ascontiguousarray(X.T).reshape((d,) + dims), y.reshape(dims)


def make(X, y, Q, isotropic, **kw):
    import gpim_amd
    Xg, yg = scattered(X, y)
    return gpim_amd.skreconstructor(Xg, yg, kernel='Spectral', n_mixtures=Q, isotropic=isotropic, verbose=0, **kw)


def engine_kmat(rec, X, Z, u):
    from gpim_amd import _lib
    dev = rec._dev
    Xd = torch.as_tensor(X, dtype=torch.float64, device=dev).contiguous()
    ud = torch.as_tensor(u, dtype=torch.float64, device=dev).contiguous()
    M = X.shape[0] if Z is None else Z.shape[0]
    out = torch.zeros((X.shape[0], M), dtype=torch.float64, device=dev)
    Zd = None if Z is None else torch.as_tensor(Z, dtype=torch.float64, device=dev).contiguous()
    _lib.check(rec._handle.lib.gpimhip_sm_kmat(rec._handle.h, ctypes.byref(rec._sstruct), _lib.ptr(Xd), X.shape[0],
                                               None if Zd is None else _lib.ptr(Zd), M, _lib.ptr(ud), _lib.ptr(out), M))
    return out.cpu().numpy()


@pytest.mark.parametrize("isotropic", [False, True])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
@pytest.mark.parametrize("Q", [1, 4, 16])
def test_kmat_matches_oracle(Q, d, isotropic):
    D = 1 if isotropic else d
    X, y = S.random_data(150, d, seed=Q + d)
    Z, _ = S.random_data(70, d, seed=100 + Q + d)
    rec = make(X, y, Q, isotropic)
    u = S.random_u(Q, D, seed=3 * Q + d)
    sw = float(np.sum(np.log1p(np.exp(u[1:1 + Q]))))
    noise = 1e-4 + float(np.log1p(np.exp(u[-1])))
    Ks = engine_kmat(rec, X, None, u)
    Ko = S.kmat(X, X, u, Q, D).numpy() + noise * np.eye(X.shape[0])
    assert np.abs(Ks - Ko).max() <= 1e-13 * sw
    Kc = engine_kmat(rec, X, Z, u)
    assert np.abs(Kc - S.kmat(X, Z, u, Q, D).numpy()).max() <= 1e-13 * sw


@pytest.mark.parametrize("isotropic", [False, True])
def test_kmat_accuracy_on_pixel_grid(isotropic):
    """The workload's regime: integer pixel coordinates up to 255 and means near 0.5 per pixel, so that the per-point phases
    2 pi m x reach ~800 rad.  Both the engine's angle addition and the oracle's cos(2 pi tau m) then carry a rounding error
    of order |phase| eps per dimension; the bound is a small multiple of that."""
    Q, d = 4, 2
    D = 1 if isotropic else d
    X, y = S.grid_data(500, 256, seed=21)
    Z, _ = S.grid_data(300, 256, seed=22)
    rec = make(X, y, Q, isotropic)
    rng = np.random.default_rng(23)
    u = S.random_u(Q, D, seed=24)
    u[1 + Q:1 + Q + Q * D] = np.log(np.expm1(rng.uniform(0.3, 0.5, Q * D)))       # means
    u[1 + Q + Q * D:1 + Q + 2 * Q * D] = np.log(np.expm1(rng.uniform(0.002, 0.02, Q * D)))   # scales: long-range terms
    m = np.log1p(np.exp(u[1 + Q:1 + Q + Q * D]))
    sw = float(np.sum(np.log1p(np.exp(u[1:1 + Q]))))
    noise = 1e-4 + float(np.log1p(np.exp(u[-1])))
    phase = 2 * np.pi * m.max() * 255.0
    tol = 8.0 * d * phase * np.finfo(np.float64).eps * sw
    Ks = engine_kmat(rec, X, None, u)
    Ko = S.kmat(X, X, u, Q, D).numpy() + noise * np.eye(X.shape[0])
    assert np.abs(Ks - Ko).max() <= tol
    assert np.abs(Ks - np.diag(np.diag(Ks))).max() > 0.1 * sw      # the long-range terms are not negligible
    Kc = engine_kmat(rec, X, Z, u)
    assert np.abs(Kc - S.kmat(X, Z, u, Q, D).numpy()).max() <= tol


NLL_CASES = [(7, 2, 4, False), (100, 2, 4, False), (129, 2, 4, True), (1000, 2, 4, False), (2000, 2, 4, False),
             (129, 1, 16, False), (300, 3, 2, False), (300, 4, 1, True), (257, 4, 5, False)]


@pytest.mark.parametrize("N,d,Q,isotropic", NLL_CASES)
def test_nll_grad_matches_oracle(N, d, Q, isotropic):
    D = 1 if isotropic else d
    X, y = S.random_data(N, d, seed=N + d)
    rec = make(X, y, Q, isotropic)
    for seed in (1, 2):
        u = S.random_u(Q, D, seed=seed + N)
        l0, g0 = S.loss_grad(u, X, y, Q, D)
        l1, g1 = rec.nll_grad(u)
        assert abs(l1 - l0) <= 1e-10 * abs(l0)
        assert np.abs(g1 - g0).max() <= 1e-10 * np.abs(g0).max()


@pytest.mark.parametrize("N,isotropic", [(90, False), (300, True)])
def test_fit_matches_oracle_trajectory(N, isotropic):
    Q, d = 3, 2
    D = 1 if isotropic else d
    X, y = S.grid_data(N, 16 if N < 200 else 24, seed=5)     # integer pixel coordinates (the initial means stay below 0.5 per pixel)
    rec = make(X, y, Q, isotropic, learning_rate=0.05, iterations=100)
    u0 = rec._u.cpu().numpy().copy()
    assert np.array_equal(u0, S.initial_raw(X, y, Q, isotropic, 0))
    rec.train()
    lo, rows, _ = S.fit(u0, X, y, Q, D, 0.05, 100)
    le = np.array(rec.loss_all)
    assert le.shape == (100,)
    assert np.all(np.abs(le - lo) <= 1e-8 * np.abs(lo))
    o, _ = __import__("gpim_amd.smgpr", fromlist=["raw_layout"]).raw_layout(Q, D)
    w = np.array(rec.hyperparams["weights"])
    sc = np.array(rec.hyperparams["scales"]).reshape(100, -1)
    me = np.array(rec.hyperparams["means"]).reshape(100, -1)
    nz = np.array(rec.hyperparams["noise"])
    assert np.allclose(w, rows[:, o["w"]], rtol=1e-8, atol=0)
    assert np.allclose(sc, 1.0 / np.sqrt(rows[:, o["s"]]), rtol=1e-8, atol=0)
    assert np.allclose(me, 1.0 / rows[:, o["m"]], rtol=1e-8, atol=0)
    assert np.allclose(nz, rows[:, -1], rtol=1e-8, atol=0)


def test_graph_replay_equals_eager_launches(monkeypatch):
    """One captured iteration replayed (default) against the same launches enqueued iteration by iteration
    (GPIMHIP_NO_GRAPH=1): the same bits in the loss and hyper-parameter histories, the raw parameters and the posterior."""
    X, y = S.grid_data(300, 24, seed=5)
    Xg, _ = scattered(X, y)
    hs = []
    for knob in (None, "1"):
        if knob:
            monkeypatch.setenv("GPIMHIP_NO_GRAPH", knob)
        else:
            monkeypatch.delenv("GPIMHIP_NO_GRAPH", raising=False)
        rec = make(X, y, 3, False, learning_rate=0.05, iterations=30)
        rec.train()
        mean, sd = rec.predict(Xg)
        hs.append((np.array(rec.loss_all), rec._u.cpu().numpy(), mean, sd, np.array(rec.hyperparams["weights"]),
                   np.array(rec.hyperparams["means"]), np.array(rec.hyperparams["scales"]), np.array(rec.hyperparams["noise"])))
    assert all(np.isfinite(a).all() for a in hs[0][:4])
    for a, b in zip(*hs):
        assert np.array_equal(a, b)


def test_predict_matches_oracle_with_nan_rows():
    check_predict_with_nan_rows(400)


@pytest.mark.parametrize("N", [400, 200])
def test_predict_in_chunks_matches_oracle_with_nan_rows(monkeypatch, N):
    """GPIMHIP_PREDICT_CHUNK=128: the 333 test rows in three chunks with a ragged last one; four and two block rows."""
    monkeypatch.setenv("GPIMHIP_PREDICT_CHUNK", "128")
    check_predict_with_nan_rows(N)


def check_predict_with_nan_rows(N):
    Q, d = 4, 2
    X, y = S.random_data(N, d, seed=9)
    Z, _ = S.random_data(333, d, seed=10)
    Z[[0, 17, 200]] = np.nan
    rec = make(X, y, Q, False)
    u = S.random_u(Q, d, seed=11)
    rec._u.copy_(torch.as_tensor(u))
    Zg = np.ascontiguousarray(Z.T).reshape(d, Z.shape[0], 1)
    mean, sd = rec.predict(Zg)
    mo, vo = S.predict(u, X, y, Z, Q, d)
    mean, sd = mean.ravel(), sd.ravel()
    nan = np.isnan(Z).any(1)
    assert np.all(np.isnan(mean[nan])) and np.all(np.isnan(sd[nan]))
    assert np.abs(mean[~nan] - mo[~nan]).max() <= 1e-10
    assert np.abs(sd[~nan] - np.sqrt(vo[~nan])).max() <= 1e-10


def test_notebook_call_shape():
    import gpim
    from problems import lattice_image
    R, _ = lattice_image(64, frac=0.25)
    assert np.isnan(R).any()
    X_sparse, X_full = gpim.utils.get_sparse_grid(R), gpim.utils.get_full_grid(R)
    rec = gpim.skreconstructor(X_sparse, R, X_full, 'Spectral', lengthscale=[[1, 1], [4, 4]], sparse=True,
                               grid_points_ratio=1., learning_rate=0.1, iterations=50, verbose=0)
    mean, sd, hyper = rec.run()
    assert mean.shape == R.shape and sd.shape == R.shape
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(sd))
    assert set(hyper) == {"scales", "means", "weights", "noise", "maxdim"}
    assert hyper["maxdim"] == max(R.shape)
    assert len(hyper["weights"]) == len(hyper["scales"]) == len(hyper["means"]) == len(hyper["noise"]) == 50
    assert hyper["weights"][0].shape == (4,) and hyper["scales"][0].shape == (4, 1, 2) and hyper["means"][0].shape == (4, 1, 2)
    assert isinstance(hyper["noise"][0], float)
    assert rec.loss_all[-1] < rec.loss_all[0]
    # two identical runs: bitwise-identical outputs
    rec2 = gpim.skreconstructor(X_sparse, R, X_full, 'Spectral', sparse=True, learning_rate=0.1, iterations=50, verbose=0)
    mean2, sd2, hyper2 = rec2.run()
    assert np.array_equal(mean, mean2) and np.array_equal(sd, sd2)
    assert np.array_equal(np.array(rec.loss_all), np.array(rec2.loss_all))
    assert np.array_equal(np.array(hyper["weights"]), np.array(hyper2["weights"]))


def test_single_precision_and_out_of_scope():
    import gpim
    X, y = S.random_data(50, 2, seed=1)
    Xg, yg = scattered(X, y)
    with pytest.raises(NotImplementedError):
        gpim.skreconstructor(Xg, yg, kernel='Spectral', precision='single', verbose=0)


def test_rbf_notebook_call_accepts_sparse_keyword():
    import gpim
    R = np.cos(np.arange(24)[:, None] / 4.0) * np.sin(np.arange(20)[None, :] / 3.0 + 0.2)
    X = gpim.utils.get_full_grid(R)
    mean, sd, hyper = gpim.skreconstructor(X, R, X, 'RBF', lengthscale=[[1., 1.], [4., 4.]], sparse=True,
                                           grid_points_ratio=1., learning_rate=0.1, iterations=5, verbose=0).run()
    assert mean.shape == R.shape and np.all(np.isfinite(mean)) and np.all(np.isfinite(sd))
