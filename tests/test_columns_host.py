"""Host-side checks of the dense-by-Kronecker blocks (gprutils.column_blocks): the detection of the
complete axes, the layout of Y and of the outputs through the axis permutation, and the formulas of csrc/pkron.hip restated
in numpy (columns_oracle.py) against float64 autograd and the dense posterior of the model on all N = N_s J observations."""
import numpy as np
import pytest
import torch

import columns_oracle as CO
from gpim_amd import gprutils

_F64 = torch.float64


_cube = CO.cube


def test_cube_xy_columns():
    Xg, X, y = _cube((6, 5, 7), (0, 1), 16.0 / 30)
    C = gprutils.column_blocks(X, y)
    assert C["ragged"] == [0, 1] and C["complete"] == [2] and C["perm"] == [0, 1, 2] and C["inv"] == [0, 1, 2]
    assert C["Xs"].shape == (14, 2) and C["Y"].shape == (14, 7) and C["n_obs"] == 98
    assert np.array_equal(C["axes_c"][0], np.arange(7.0))
    # rows in ragged-grid order, the spectrum along each row
    obs = np.flatnonzero(~np.isnan(y[:, :, 0]).ravel())
    assert np.array_equal(C["obs"], obs)
    assert np.array_equal(C["Xs"], Xg[:2, :, :, 0].reshape(2, -1).T[obs])
    assert np.array_equal(C["Y"], y.reshape(30, 7)[obs])


def test_cube_spectral_axis_first():
    Xg, X, y = _cube((7, 6, 5), (1, 2), 16.0 / 30)
    C = gprutils.column_blocks(X, y)
    assert C["ragged"] == [1, 2] and C["complete"] == [0] and C["perm"] == [1, 2, 0] and C["inv"] == [2, 0, 1]
    assert C["Xs"].shape == (14, 2) and C["Y"].shape == (14, 7)
    # the same data as the cube with the spectral axis last
    C2 = gprutils.column_blocks(np.moveaxis(X, 1, -1)[[1, 2, 0]], np.moveaxis(y, 0, -1))
    assert np.array_equal(C["Xs"], C2["Xs"]) and np.array_equal(C["Y"], C2["Y"])
    assert np.array_equal(C["axes_c"][0], C2["axes_c"][0])


def test_four_d_two_complete_axes():
    Xg, X, y = _cube((6, 5, 4, 3), (0, 1), 0.4, seed=1)
    C = gprutils.column_blocks(X, y)
    assert C["ragged"] == [0, 1] and C["complete"] == [2, 3]
    assert C["Xs"].shape == (18, 2) and C["Y"].shape == (18, 12)
    assert [len(c) for c in C["axes_c"]] == [4, 3]
    obs = C["obs"]
    assert np.array_equal(C["Y"], y.reshape(30, 12)[obs])


def test_image_with_missing_rows():
    axes = [np.linspace(0.0, 4.5, 10), np.arange(8.0) * 0.5]
    Xg, X, y = _cube((10, 8), (0,), 0.3, seed=2, axes=axes)
    C = gprutils.column_blocks(X, y)
    assert C["ragged"] == [0] and C["complete"] == [1]
    assert C["Xs"].shape == (7, 1) and C["Y"].shape == (7, 8)
    assert np.array_equal(C["axes_c"][0], axes[1])
    assert np.array_equal(C["Xs"][:, 0], axes[0][C["obs"]])


def test_rejections():
    rng = np.random.default_rng(3)
    # scattered NaN: the mask is constant along no axis
    Xg, X, y = _cube((6, 5, 7), (0, 1), 0.0)
    for f in rng.choice(y.size, size=20, replace=False):
        idx = np.unravel_index(f, y.shape)
        y[idx] = np.nan
        X[(slice(None),) + idx] = np.nan
    with pytest.raises(NotImplementedError, match="no axis"):
        gprutils.column_blocks(X, y)
    # nothing missing: the Kronecker solver's case
    Xg, X, y = _cube((6, 5, 7), (0, 1), 0.0)
    with pytest.raises(NotImplementedError, match="Kronecker"):
        gprutils.column_blocks(X, y)
    # not a product grid along the complete axis
    Xg, X, y = _cube((6, 5, 7), (0, 1), 0.5)
    i, j = np.argwhere(~np.isnan(y[:, :, 0]))[0]
    X[2, i, j, 3] += 0.25
    with pytest.raises(NotImplementedError, match="product grid"):
        gprutils.column_blocks(X, y)
    # the NaN patterns of X and y differ
    Xg, X, y = _cube((6, 5, 7), (0, 1), 0.5)
    i, j = np.argwhere(~np.isnan(y[:, :, 0]))[0]
    y[i, j, :] = np.nan
    with pytest.raises(NotImplementedError, match="NaN pattern"):
        gprutils.column_blocks(X, y)
    # too many blocks for the batched engine
    shape = (3, 300, 300)
    yb = np.zeros(shape)
    yb[1] = np.nan
    Xb = np.array(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"))
    Xb[:, 1] = np.nan
    with pytest.raises(NotImplementedError, match="65535"):
        gprutils.column_blocks(Xb, yb)


def test_column_flops():
    assert gprutils.column_flops(301, 102) == 102 * 301.0 ** 3
    # the shipped cube's shape: J^2 below the dense model of the same observations
    assert gprutils.column_flops(301, 102) * 102 ** 2 == pytest.approx((301.0 * 102) ** 3)
    assert gprutils.column_flops(301, 102) < gprutils.border_flops(32 * 32 * 102, (1024 - 301) * 102, 3)[1]


@pytest.mark.parametrize("shape,cols", [((6, 5, 7), (0, 1)), ((7, 6, 5), (1, 2)), ((6, 5, 4, 3), (0, 1)), ((10, 8), (0,))])
def test_round_trip_through_the_permutation(shape, cols):
    Xg, X, y = _cube(shape, cols, 0.4, seed=4)
    C = gprutils.column_blocks(X, y)
    # Y back into the grid: rows at the observed ragged points, permuted axes back in place
    rshape = [shape[i] for i in C["ragged"]]
    full = np.full((int(np.prod(rshape)), C["Y"].shape[1]), np.nan)
    full[C["obs"]] = C["Y"]
    back = full.reshape([shape[i] for i in C["perm"]]).transpose(C["inv"])
    assert np.array_equal(np.isnan(back), np.isnan(y)) and np.array_equal(back[~np.isnan(y)], y[~np.isnan(y)])
    # an output on (ragged rows) x (complete axes) goes back the same way: the coordinates themselves
    taxes = [np.unique(Xg[i]) for i in range(len(shape))]
    rows = np.array(np.meshgrid(*[taxes[i] for i in C["ragged"]], indexing="ij")).reshape(len(rshape), -1).T
    for a in range(len(shape)):
        if a in C["ragged"]:
            out = np.repeat(rows[:, C["ragged"].index(a)][:, None], C["Y"].shape[1], axis=1)
        else:
            cgrid = np.array(np.meshgrid(*C["axes_c"], indexing="ij"))[C["complete"].index(a)].ravel()
            out = np.repeat(cgrid[None, :], len(rows), axis=0)
        assert np.array_equal(out.reshape([shape[i] for i in C["perm"]]).transpose(C["inv"]), Xg[a])


def _dense_torch(Xfull, yfull, var, ls, noise, jitter):
    a = Xfull / ls
    r2 = ((a[:, None, :] - a[None, :, :]) ** 2).sum(-1)
    A = var * torch.exp(-0.5 * r2) + (noise + jitter) * torch.eye(len(Xfull), dtype=_F64)
    L = torch.linalg.cholesky(A)
    al = torch.cholesky_solve(yfull[:, None], L)[:, 0]
    nll = 0.5 * (yfull * al).sum() + torch.log(torch.diagonal(L)).sum() + 0.5 * len(yfull) * CO.LOG2PI
    return nll, L, al


ORACLE_CASES = {
    "ard": ([1.3, 2.1, 1.7], False),
    "isotropic": ([1.6, 1.6, 1.6], True),
    "clamped": ([1.3, 2.1, 60.0], False),         # l_c = 60 on a 7-point axis: all but two or three lambda_j at rounding level
}


@pytest.mark.parametrize("name", sorted(ORACLE_CASES))
def test_oracle_against_dense_autograd(name):
    ls0, iso = ORACLE_CASES[name]
    Xg, X, y = _cube((6, 5, 7), (0, 1), 16.0 / 30, seed=5)
    C = gprutils.column_blocks(X, y)
    assert C["Xs"].shape[0] == 14
    jitter, var0, noise0 = 1e-5, 0.8, 0.05
    loss, dvar, dls_r, dls_c, dnoise = CO.loss_grad(C["Xs"], C["axes_c"], C["Y"], var0, np.array(ls0[:2]), np.array(ls0[2:]),
                                                    noise0, jitter)
    if name == "clamped":
        lam = np.linalg.eigvalsh(CO.rbf(C["axes_c"][0][:, None], C["axes_c"][0][:, None], np.array([60.0])))
        assert (lam < 1e-9).sum() >= 3
    obs = ~np.isnan(y).ravel()
    Xf = torch.from_numpy(Xg.reshape(3, -1).T[obs].copy())
    yf = torch.from_numpy(y.ravel()[obs].copy())
    var = torch.tensor(var0, dtype=_F64, requires_grad=True)
    noise = torch.tensor(noise0, dtype=_F64, requires_grad=True)
    if iso:
        l1 = torch.tensor(ls0[0], dtype=_F64, requires_grad=True)
        ls = l1 * torch.ones(3, dtype=_F64)
    else:
        l1 = torch.tensor(ls0, dtype=_F64, requires_grad=True)
        ls = l1
    nll, L, al = _dense_torch(Xf, yf, var, ls, noise, jitter)
    gv, gl, gn = torch.autograd.grad(nll, [var, l1, noise])
    got_l = np.concatenate([dls_r, dls_c])
    got = np.concatenate([[dvar], [got_l.sum()] if iso else got_l, [dnoise]])
    want = np.concatenate([[gv.item()], np.atleast_1d(gl.numpy()), [gn.item()]])
    scale = np.abs(want).max()
    print(name, "loss dev %.2e, gradient max abs dev %.2e (largest component %.3g)"
          % (abs(loss - nll.item()), np.abs(got - want).max(), scale))
    assert abs(loss - nll.item()) <= 1e-10 * abs(nll.item())
    assert np.abs(got - want).max() <= 1e-10 * scale
    # posterior on the full grid with a 2x finer spectral axis against the dense posterior
    ct = np.arange(0.0, 6.01, 0.5)
    rows = Xg[:2, :, :, 0].reshape(2, -1).T
    mean, v = CO.predict(C["Xs"], C["axes_c"], C["Y"], var0, np.array(ls0[:2]), np.array(ls0[2:]), noise0, jitter, rows, [ct])
    Xt = np.concatenate([np.repeat(rows, len(ct), axis=0), np.tile(ct, len(rows))[:, None]], axis=1)
    with torch.no_grad():
        a, b = Xf / ls, torch.from_numpy(Xt) / ls
        Kx = var * torch.exp(-0.5 * ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1))
        md = Kx.T @ al
        w = torch.linalg.solve_triangular(L, Kx, upper=False)
        vd = var - (w * w).sum(0) + noise
    print(name, "mean dev %.2e, variance dev %.2e" % (np.abs(mean.ravel() - md.numpy()).max(), np.abs(v.ravel() - vd.numpy()).max()))
    assert np.abs(mean.ravel() - md.numpy()).max() <= 1e-10 * max(1.0, np.abs(md.numpy()).max())
    assert np.abs(v.ravel() - vd.numpy()).max() <= 1e-10


def test_symbols_in_header_and_binding():
    from gpim_amd import _lib
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpimhip.h")).read()
    for s in ("gpimhip_pkron_nll_grad", "gpimhip_fit_pkron", "gpimhip_predict_pkron"):
        assert s in text and s in _lib.EXPORTS


def test_solver_choice_is_host_logic():
    from gpim_amd.skgpr import skreconstructor
    Xg, X, y = _cube((12, 12, 6), (0, 1), 0.4, seed=6)
    solver, C = skreconstructor._choose_solver(X, y, "RBF")
    assert solver == "columns" and C["Y"].shape[1] == 6
    # another kernel does not factorise; scattered NaN have no complete axis; a complete cube is the Kronecker solver's
    assert skreconstructor._choose_solver(X, y, "Matern52")[0] in ("border", "dense")
    assert skreconstructor._choose_solver(Xg, np.nan_to_num(y), "RBF")[0] == "kronecker"
    ys = np.nan_to_num(y)
    ys.ravel()[np.random.default_rng(7).choice(ys.size, size=40, replace=False)] = np.nan
    Xs = Xg.copy()
    Xs[:, np.isnan(ys)] = np.nan
    assert skreconstructor._choose_solver(Xs, ys, "RBF")[0] in ("border", "dense")
