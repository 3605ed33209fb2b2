"""skreconstructor on grids whose missing points are whole columns: the dense-by-Kronecker blocks (csrc/pkron.hip, DESIGN.md
section 22) against the dense exact GP on the same observed points."""
import ctypes

import numpy as np
import pytest
import torch

import gpim_amd
from columns_oracle import cube
from gpim_amd import _lib
from gpim_amd._lib import ptr

pytestmark = pytest.mark.gpu

CUBES = {
    "12x12x6": ((12, 12, 6), (0, 1), 0.4, 2),          # N_s = 86: one block column
    "16x16x5": ((16, 16, 5), (0, 1), 0.35, 3),         # N_s = 166 > 128: two block columns, a ragged last one
    "6x5x4x3": ((6, 5, 4, 3), (0, 1), 0.4, 1),         # two complete axes
    "5x12x12": ((5, 12, 12), (1, 2), 0.4, 4),          # spectral axis first: through the permutation
}
_made = {}


def _data(name):
    if name not in _made:
        shape, cols, frac, seed = CUBES[name]
        _made[name] = cube(shape, cols, frac, seed=seed)
    return _made[name]


def _pair(name, **kw):
    Xg, X, R = _data(name)
    kw = dict(dict(learning_rate=0.1, iterations=1, verbose=0), **kw)
    b = gpim_amd.skreconstructor(X, R, Xg, kernel="RBF", **kw)
    d = gpim_amd.reconstructor(X, R, Xg, kernel="RBF", **kw)
    return b, d, Xg


@pytest.mark.parametrize("iso", [False, True], ids=["ard", "isotropic"])
@pytest.mark.parametrize("name", sorted(CUBES))
def test_loss_grad_parity(name, iso):
    b, d, _ = _pair(name, isotropic=True) if iso else _pair(name)
    assert b.solver == "columns", name
    ns = {"12x12x6": 86, "16x16x5": 166, "6x5x4x3": 18, "5x12x12": 86}[name]
    assert b._solver.C["Xs"].shape[0] == ns
    d._u.copy_(b._u)
    lb, gb = b.loss_and_grad()
    ld, gd = d.loss_and_grad()
    rel = ((gb - gd).abs() / gd.abs().clamp(min=1e-300)).max().item()
    print("%s %s: loss %.12g rel dev %.2e, gradient max rel dev %.2e" % (name, "iso" if iso else "ard", ld, abs(lb - ld) / abs(ld), rel))
    assert abs(lb - ld) <= 1e-9 * abs(ld), (lb, ld)
    assert rel <= 1e-9, (gb, gd)


@pytest.fixture(scope="module")
def trained():
    b, d, Xg = _pair("16x16x5", iterations=30)
    return b, d, b.run(), d.run()


def test_training_and_prediction_match_dense(trained):
    b, d, (mb, sb, hb), (md, sd, hd) = trained
    assert b.solver == "columns"
    for key in ("lengthscale", "noise", "variance"):
        assert np.allclose(np.asarray(hb[key]), np.asarray(hd[key]), rtol=1e-6, atol=0), key
    assert len(b.loss_all) == 30 and np.allclose(b.loss_all, d.loss_all, rtol=1e-6, atol=0)
    print("max |mean| dev %.2e, max |sd| dev %.2e" % (np.abs(mb - md).max(), np.abs(sb - sd).max()))
    assert mb.shape == (16, 16, 5) and np.abs(mb - md).max() < 1e-7 and np.abs(sb - sd).max() < 1e-7


def test_prediction_on_a_finer_grid(trained):
    b, d = trained[0], trained[1]
    Xh = gpim_amd.utils.get_full_grid(_data("16x16x5")[2], dense_x=0.5)
    mb2, sb2 = b.predict(Xh)
    md2, sd2 = d.predict(Xh)
    print("dense_x=0.5: max |mean| dev %.2e, max |sd| dev %.2e" % (np.abs(mb2 - md2).max(), np.abs(sb2 - sd2).max()))
    assert mb2.shape == Xh.shape[1:] and np.abs(mb2 - md2).max() < 1e-7 and np.abs(sb2 - sd2).max() < 1e-7


def test_predict_at_rows(trained):
    # rows that form a product grid (a crop of the cube) are served; anything else is refused with the reason
    b, d = trained[0], trained[1]
    Xg = _data("16x16x5")[0]
    rows = Xg[:, 2:6, 3:5, :].reshape(3, -1).T.copy()
    # (any set of pixels) x (the spectral axis), in any order: one pixel dropped with its spectrum, the rows shuffled
    rows = rows[5:][np.random.default_rng(0).permutation(len(rows) - 5)]
    rows = torch.from_numpy(rows.copy()).to(b._dev)
    mb, sb = b._predict_device(rows)
    md, sd = d._predict_device(rows)
    assert (mb - md).abs().max().item() < 1e-7 and (sb - sd).abs().max().item() < 1e-7
    with pytest.raises(NotImplementedError, match="product"):
        b._predict_device(rows[:-1].contiguous())


def test_bitwise_repeatable():
    outs = []
    for _ in range(2):
        b = _pair("5x12x12", iterations=12)[0]
        m, s, h = b.run()
        outs.append((m, s, np.asarray(b.loss_all), np.asarray(h["lengthscale"])))
    for a, c in zip(outs[0], outs[1]):
        assert np.array_equal(a, c)


def test_solver_choice():
    Xg, X, R = _data("12x12x6")
    rec = gpim_amd.skreconstructor(X, R, Xg, kernel="RBF", verbose=0)
    assert rec.solver == "columns" and rec.do_structured
    with pytest.raises(NotImplementedError):
        rec.model.y = rec.model.y
    # posterior draws are not built for this solver
    for method in ("joint", "pathwise", "blocks", "border", "kron"):
        with pytest.raises(NotImplementedError, match="columns"):
            rec.sample(1, method=method)
    # scattered NaN: no complete axis -- today's choice
    Rs = np.nan_to_num(R)
    Rs.ravel()[np.random.default_rng(0).choice(Rs.size, size=60, replace=False)] = np.nan
    Xs = Xg.copy()
    Xs[:, np.isnan(Rs)] = np.nan
    assert gpim_amd.skreconstructor(Xs, Rs, Xg, kernel="RBF", verbose=0).solver in ("border", "dense")
    # another kernel does not factorise over the complete axis
    assert gpim_amd.skreconstructor(X, R, Xg, kernel="Matern52", verbose=0).solver in ("border", "dense")
    # the complete cube stays with the Kronecker solver
    assert gpim_amd.skreconstructor(Xg, np.nan_to_num(R), Xg, kernel="RBF", verbose=0).solver == "kronecker"
    # reconstructor(structured=True) keeps refusing NaN
    with pytest.raises(NotImplementedError):
        gpim_amd.reconstructor(X, R, Xg, kernel="RBF", structured=True, verbose=0)


def test_cabi_misuse_leaves_the_handle_usable():
    Xg, X, R = _data("12x12x6")
    rec = gpim_amd.skreconstructor(X, R, Xg, kernel="RBF", verbose=0)
    sol, lib = rec._solver, rec._handle.lib
    out = torch.empty(1 + rec._u.numel(), dtype=torch.float64, device=rec._dev)
    lg = (ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(out.data_ptr() + 8))
    args = lambda h, m, n_c, p=2: (h, ctypes.byref(m), ptr(sol.Xs_d), sol.Xs_d.shape[0], p, 3 - p, n_c, sol.perm,
                                   ptr(sol.axes_d), ptr(sol.Y_d), ptr(rec._u), *lg)
    good, _ = rec.loss_and_grad()
    # another kernel
    m52 = gpim_amd.kernels.get_kernel("Matern52", 3, [[0.] * 3, [5.] * 3]).struct()
    assert lib.gpimhip_pkron_nll_grad(*args(rec._handle.h, m52, sol.n_c)) == _lib.E_BADARG
    assert "RBF" in lib.gpimhip_last_error().decode()
    # more blocks than the batched engine takes (refused before anything is read)
    big = (ctypes.c_int32 * 2)(300, 300)
    assert lib.gpimhip_pkron_nll_grad(*args(rec._handle.h, rec._mstruct, big, p=1)) == _lib.E_BADARG
    assert "65535" in lib.gpimhip_last_error().decode()
    # a single-precision handle
    H32 = _lib.Handle(precision="single")
    assert lib.gpimhip_pkron_nll_grad(*args(H32.h, rec._mstruct, sol.n_c)) == _lib.E_BADARG
    again, _ = rec.loss_and_grad()
    assert again == good
