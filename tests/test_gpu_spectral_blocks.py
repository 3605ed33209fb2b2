"""The spectral-mixture GP of skreconstructor(kernel='Spectral') on reflection blocks and bordered blocks on the MI355X
(include/gpimhip.h: gpimhip_*_sm_batched).  The oracle is the dense float64 restatement of
tests/sm_oracle.py on the flattened observed points; the block covariance alone is compared with the entry-by-entry
restatement of tests/sm_blocks_oracle.py."""
import ctypes

import numpy as np
import pytest
import torch

import sm_blocks_oracle as SB
import sm_oracle as S

pytestmark = pytest.mark.gpu

NONUNIFORM = [np.arange(12.0), np.array([0.0, 0.7, 1.9, 3.0, 3.6, 5.1, 6.0, 7.4, 8.0])]


def image(shape, seed, missing=0, forced=(), axes=None):
    """(X, y) of the reconstructor: a quasi-periodic image on the grid, NaN at the missing pixels in both."""
    X = SB.grid(shape, axes)
    y = SB.smooth_image(shape, seed)
    if missing:
        y = SB.punch(y, missing, seed=seed + 100, forced=forced)
        X = SB.with_holes(X, y)
    return X, y


def make(X, y, Q, isotropic=False, **kw):
    import gpim_amd
    return gpim_amd.skreconstructor(X, y, kernel='Spectral', n_mixtures=Q, isotropic=isotropic, verbose=0, **kw)


def engine_block_kmat(rec, Z, u):
    """gpimhip_sm_kmat on the handle in reflection mode: (B, Nq, Nq) or (B, Nq, M)."""
    from gpim_amd import _lib
    ud = torch.as_tensor(u, dtype=torch.float64, device=rec._dev).contiguous()
    Zd = None if Z is None else torch.as_tensor(Z, dtype=torch.float64, device=rec._dev).contiguous()
    with rec._solver._mode(rec) as D:
        Nq = D.Xq.shape[0]
        M = Nq if Z is None else Z.shape[0]
        out = torch.full((D.B * Nq, M), np.nan, dtype=torch.float64, device=rec._dev)
        _lib.check(rec._handle.lib.gpimhip_sm_kmat(rec._handle.h, ctypes.byref(rec._sstruct), _lib.ptr(D.Xq), Nq,
                                                   None if Zd is None else _lib.ptr(Zd), M, _lib.ptr(ud), _lib.ptr(out), M))
        return out.cpu().numpy().reshape(D.B, Nq, M)


# ------------------------------------------------------------------ 1. the block covariance
@pytest.mark.parametrize("isotropic", [False, True])
@pytest.mark.parametrize("Q", [1, 4, 16])
@pytest.mark.parametrize("shape", [(13, 10), (24, 24), (6, 5, 4)])
def test_block_kmat_matches_restatement(shape, Q, isotropic):
    d = len(shape)
    D = 1 if isotropic else d
    X, y = image(shape, seed=Q)
    rec = make(X, y, Q, isotropic)
    assert rec.solver == "reflection"
    B = SB.blocks_of(X, y)
    u = S.random_u(Q, D, seed=5 * Q + d)
    sw = float(np.sum(np.log1p(np.exp(u[1:1 + Q]))))
    rng = np.random.default_rng(Q + d)
    Z = rng.uniform(-1.0, max(shape), size=(70, d))
    Ks = engine_block_kmat(rec, None, u)
    Kc = engine_block_kmat(rec, Z, u)
    assert Ks.shape[0] == B["B"] == 2 ** d
    es = max(np.abs(Ks[b] - SB.block_kmat(B, b, u, Q, D).numpy()).max() for b in range(B["B"]))
    ec = max(np.abs(Kc[b] - SB.block_kmat(B, b, u, Q, D, Z).numpy()).max() for b in range(B["B"]))
    print("block kmat", shape, Q, isotropic, "sym %.3e cross %.3e bound %.3e" % (es, ec, 1e-13 * sw))
    assert es <= 1e-13 * sw
    assert ec <= 1e-13 * sw


# ------------------------------------------------------------------ 2. / 3. loss and gradient
def check_nll(X, y, Q, isotropic, solver, blocks):
    D = 1 if isotropic else X.shape[0]
    rec = make(X, y, Q, isotropic)
    assert rec.solver == solver and rec._solver.S["B"] == blocks
    Xf, yf = SB.flat(X, y)
    for seed in (1, 2):
        u = S.random_u(Q, D, seed=seed + 11 * Q + yf.size)
        l0, g0 = S.loss_grad(u, Xf, yf, Q, D)
        l1, g1 = rec.nll_grad(u)
        print("nll", y.shape, solver, "dloss %.3e dgrad %.3e" % (abs(l1 - l0) / abs(l0), np.abs(g1 - g0).max() / np.abs(g0).max()))
        assert abs(l1 - l0) <= 1e-9 * abs(l0)
        assert np.abs(g1 - g0).max() <= 1e-9 * np.abs(g0).max()


COMPLETE = [((12, 10), 4, False, None, 4), ((13, 10), 3, True, None, 4), ((13, 11), 2, False, None, 4),
            ((24, 24), 4, False, None, 4), ((6, 5, 4), 2, False, None, 8), ((4, 4, 3, 2), 1, False, None, 16),
            ((40,), 16, False, None, 2), ((12, 9), 3, False, NONUNIFORM, 2)]


@pytest.mark.parametrize("shape,Q,isotropic,axes,blocks", COMPLETE)
def test_nll_grad_on_complete_grids(shape, Q, isotropic, axes, blocks):
    X, y = image(shape, seed=len(shape) + Q, axes=axes)
    check_nll(X, y, Q, isotropic, "reflection", blocks)


BORDERED = [((16, 16), 1, (), 4), ((16, 16), 13, (), 4), ((15, 16), 20, (7 * 16 + 3,), 4), ((6, 5, 4), 6, (), 8)]


@pytest.mark.parametrize("shape,missing,forced,blocks", BORDERED)
def test_nll_grad_with_a_border(shape, missing, forced, blocks):
    X, y = image(shape, seed=missing, missing=missing, forced=forced)
    assert np.isnan(y).sum() == missing and all(np.isnan(y.reshape(-1)[i]) for i in forced)
    check_nll(X, y, 3, False, "border", blocks)


# ------------------------------------------------------------------ 4. training
@pytest.mark.parametrize("shape,isotropic,missing", [((16, 16), False, 0), ((15, 16), True, 0), ((16, 16), False, 13)])
def test_thirty_iterations_match_oracle_trajectory(shape, isotropic, missing):
    from gpim_amd.smgpr import raw_layout
    Q, T = 3, 30
    D = 1 if isotropic else 2
    X, y = image(shape, seed=7, missing=missing)
    rec = make(X, y, Q, isotropic, learning_rate=0.05, iterations=T)
    assert rec.solver == ("border" if missing else "reflection")
    Xf, yf = SB.flat(X, y)
    u0 = rec._u.cpu().numpy().copy()
    assert np.array_equal(u0, S.initial_raw(Xf, yf, Q, isotropic, 0))
    rec.train()
    lo, rows, _ = S.fit(u0, Xf, yf, Q, D, 0.05, T)
    le = np.array(rec.loss_all)
    assert le.shape == (T,)
    o, _ = raw_layout(Q, D)
    w = np.array(rec.hyperparams["weights"])
    sc = np.array(rec.hyperparams["scales"]).reshape(T, -1)
    me = np.array(rec.hyperparams["means"]).reshape(T, -1)
    nz = np.array(rec.hyperparams["noise"])
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.abs(b)))
    print("fit", shape, missing, "loss %.3e w %.3e s %.3e m %.3e noise %.3e" % (
        rel(le, lo), rel(w, rows[:, o["w"]]), rel(sc, 1.0 / np.sqrt(rows[:, o["s"]])), rel(me, 1.0 / rows[:, o["m"]]),
        rel(nz, rows[:, -1])))
    assert np.all(np.abs(le - lo) <= 1e-8 * np.abs(lo))
    assert np.allclose(w, rows[:, o["w"]], rtol=1e-8, atol=0)
    assert np.allclose(sc, 1.0 / np.sqrt(rows[:, o["s"]]), rtol=1e-8, atol=0)
    assert np.allclose(me, 1.0 / rows[:, o["m"]], rtol=1e-8, atol=0)
    assert np.allclose(nz, rows[:, -1], rtol=1e-8, atol=0)


# ------------------------------------------------------------------ 5. prediction
@pytest.mark.parametrize("missing", [0, 13])
def test_predict_matches_oracle(missing):
    check_predict(missing, (16, 15))


@pytest.mark.parametrize("missing", [0, 13])
def test_predict_in_chunks_matches_oracle(monkeypatch, missing):
    """GPIMHIP_PREDICT_CHUNK=128 on a 16 x 16 grid reflected in both axes (64-point blocks, B = 4): on the training grid the
    variance is wanted for the first 64 points, so chunk 1 has nvar < cnt and chunk 2 nvar == 0 (with a border: all of it)."""
    monkeypatch.setenv("GPIMHIP_PREDICT_CHUNK", "128")
    check_predict(missing, (16, 16))


def check_predict(missing, shape):
    import gpim_amd
    Q = 3
    X, y = image(shape, seed=9, missing=missing)
    rec = make(X, y, Q)
    assert rec.solver == ("border" if missing else "reflection")
    u = S.random_u(Q, 2, seed=12)
    rec._u.copy_(torch.as_tensor(u))
    Xf, yf = SB.flat(X, y)
    rng = np.random.default_rng(13)
    Z = rng.uniform(-1.0, 17.0, size=(50, 2))
    Z[[3, 41]] = np.nan
    full = gpim_amd.utils.get_full_grid(y)
    fine = gpim_amd.utils.get_full_grid(y, dense_x=0.5)
    for name, grid in (("training grid", full), ("dense_x=0.5", fine), ("off-grid rows", np.ascontiguousarray(Z.T).reshape(2, 50, 1))):
        mean, sd = rec.predict(grid)
        assert mean.shape == grid.shape[1:] == sd.shape
        rows = grid.reshape(2, -1).T
        mo, vo = S.predict(u, Xf, yf, rows, Q, 2)
        mean, sd = mean.ravel(), sd.ravel()
        nan = np.isnan(rows).any(1)
        assert nan.sum() == (2 if name == "off-grid rows" else 0)
        assert np.all(np.isnan(mean[nan])) and np.all(np.isnan(sd[nan]))
        print("predict", missing, name, "mean %.3e sd %.3e" % (np.abs(mean[~nan] - mo[~nan]).max(),
                                                               np.abs(sd[~nan] - np.sqrt(vo[~nan])).max()))
        assert np.abs(mean[~nan] - mo[~nan]).max() <= 1e-9
        assert np.abs(sd[~nan] - np.sqrt(vo[~nan])).max() <= 1e-9


# ------------------------------------------------------------------ 6. the public surface
def test_solver_reported_for_the_three_regimes():
    import gpim
    X, y = image((16, 16), seed=3)
    assert gpim.skreconstructor(X, y, kernel='Spectral', verbose=0).solver == "reflection"
    X5, y5 = image((16, 16), seed=3, missing=5)
    assert gpim.skreconstructor(X5, y5, kernel='Spectral', verbose=0).solver == "border"
    Xh, yh = image((16, 16), seed=3, missing=192)
    assert gpim.skreconstructor(Xh, yh, kernel='Spectral', verbose=0).solver == "dense"
    assert gpim.skreconstructor(X, y, kernel='Spectral', verbose=0, solver="dense").solver == "dense"
    with pytest.raises(NotImplementedError):
        gpim.skreconstructor(X, y, kernel='Spectral', verbose=0, solver="border")


def run(X, y, **kw):
    import gpim
    rec = gpim.skreconstructor(X, y, gpim.utils.get_full_grid(y), 'Spectral', learning_rate=0.05, iterations=20, verbose=0, **kw)
    mean, sd, hyper = rec.run()
    return rec, mean, sd, hyper


def test_default_agrees_with_forced_dense_and_repeats_bitwise():
    X, y = image((16, 16), seed=4)
    rb, mb, sb, hb = run(X, y)
    rd, md, sdd, hd = run(X, y, solver="dense")
    assert (rb.solver, rd.solver) == ("reflection", "dense")
    assert set(hb) == set(hd) and len(hb["weights"]) == 20 and hb["scales"][0].shape == hd["scales"][0].shape
    lb, ld = np.array(rb.loss_all), np.array(rd.loss_all)
    print("blocks vs dense: mean %.3e sd %.3e loss %.3e" % (np.abs(mb - md).max(), np.abs(sb - sdd).max(),
                                                           np.max(np.abs(lb - ld) / np.abs(ld))))
    assert np.abs(mb - md).max() <= 1e-8 and np.abs(sb - sdd).max() <= 1e-8
    assert np.all(np.abs(lb - ld) <= 1e-8 * np.abs(ld))
    r2, m2, s2, h2 = run(X, y)
    assert np.array_equal(mb, m2) and np.array_equal(sb, s2) and np.array_equal(lb, np.array(r2.loss_all))
    assert np.array_equal(np.array(hb["means"]), np.array(h2["means"]))


def test_graph_replay_equals_eager_launches_with_a_border(monkeypatch):
    X, y = image((16, 16), seed=5, missing=13)
    outs = []
    for knob in (None, "1"):
        if knob:
            monkeypatch.setenv("GPIMHIP_NO_GRAPH", knob)
        else:
            monkeypatch.delenv("GPIMHIP_NO_GRAPH", raising=False)
        rec, mean, sd, hyper = run(X, y)
        assert rec.solver == "border"
        outs.append((np.array(rec.loss_all), rec._u.cpu().numpy(), mean, sd, np.array(hyper["weights"]),
                     np.array(hyper["means"]), np.array(hyper["scales"]), np.array(hyper["noise"])))
    assert all(np.isfinite(a).all() for a in outs[0])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
