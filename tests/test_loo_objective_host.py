"""
The leave-one-out objective without a GPU: the two float64 references of
tests/loo_objective_oracle.py against each other and against the definition, the new C-ABI symbols, and the Python refusals
that need no device.
"""
import ctypes
import math

import numpy as np
import pytest
import torch
from numpy.testing import assert_allclose

import loo_objective_oracle as LG
import loo_oracle as LO


@pytest.mark.parametrize("kind,N,d,iso", LG.CASES)
def test_closed_form_matches_autograd(kind, N, d, iso):
    """The G2 / r gradient (the engine's arithmetic, kernel derivatives by hand) against torch autograd through an explicit
    inverse, at the GPU test's bar: loss rtol 1e-12, gradient rtol 1e-10 / atol 1e-10.  Prints the spread of the two
    references -- what the GPU test's bar is judged against (measured: loss <= 1.7e-14 relative, gradient <= 3.5e-12 absolute
    on entries up to 133, on every case below a tenth of the bar)."""
    kp, _, _, X, y = LO.problem(kind, N, d, iso)
    ref = LG.reference(kind, N, d, iso)
    got = LG.closed(kp, X, y)
    rel, ab = LG.spread(got, ref)
    print("spread %s N=%d d=%d iso=%s: loss rel %.2e, grad abs %.2e (|grad| max %.2e)" % (kind, N, d, iso, rel, ab,
                                                                                        np.abs(ref[1]).max()))
    assert_allclose(got[0], ref[0], rtol=1e-12)
    assert_allclose(got[1], ref[1], rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("kind,N,d,iso", [c for c in LG.CASES if c[1] <= 130])
def test_loss_is_negated_elpd_of_refits(kind, N, d, iso):
    """loss - prior constant = -sum_i log N(y_i | mean_i, var_i + jitter) over N brute-force refits: the held-out variance
    of the trained matrix is the reported one plus the jitter (no clamp on these cases)."""
    kp, _, _, X, y = LO.problem(kind, N, d, iso)
    mean, var = LO.brute(kp, X, y)
    with torch.no_grad():
        assert (var > kp.noise.item()).all()            # nothing clamped
        prior = kp.neg_log_prior().item()
    elpd, _ = LO.score(mean, var + LO.JITTER, y.numpy())
    loss, _ = LG.closed(kp, X, y)
    assert_allclose(loss - prior, -elpd, rtol=1e-10)


def test_adam_paths_of_two_references_agree():
    """What the GPU trajectory test's bars (history rtol 1e-8, loss rtol 1e-10) stand on: 200 Adam steps on autograd's loss
    through an explicit inverse and through a Cholesky solve differ by orders less."""
    X, y = LO.scattered(60, 2, seed=3)
    ls = [[0.5, 0.5], [12., 12.]]

    def loss_chol(kp, X, y, jitter):
        N = X.shape[0]
        L = torch.linalg.cholesky(kp.K(X) + (kp.noise + jitter) * torch.eye(N, dtype=torch.float64))
        Li = torch.linalg.solve_triangular(L, torch.eye(N, dtype=torch.float64), upper=False)
        alpha, d = Li.T @ (Li @ y), (Li * Li).sum(0)
        return (-0.5 * d.log() + 0.5 * alpha * alpha / d).sum() + 0.5 * N * math.log(2.0 * math.pi) + kp.neg_log_prior()

    paths = []
    for fn in (None, loss_chol):
        torch.manual_seed(0)
        kp = LG.LO.O.KernelParams("RBF", 2, ls)
        paths.append(LG.adam_path(kp, X, y, 0.05, 200, jitter=1e-6, loss_fn=fn))
    dh = np.abs(paths[0][0] / paths[1][0] - 1.0).max()
    dl = np.abs(paths[0][1] / paths[1][1] - 1.0).max()
    print("two references over 200 Adam steps: history %.2e, loss %.2e relative; min |loss| %.3f"
          % (dh, dl, np.abs(paths[0][1]).min()))
    assert dh < 1e-10 and dl < 1e-11


def test_library_exports_the_new_entries(ensure_built):
    lib = ctypes.CDLL(ensure_built)
    for s in ("gpimhip_loo_grad", "gpimhip_fit_exact_loo"):
        assert hasattr(lib, s), "libgpimhip.so does not export %s" % s
    from gpim_amd import _lib
    assert "gpimhip_loo_grad" in _lib.EXPORTS and "gpimhip_fit_exact_loo" in _lib.EXPORTS


def _image(shape=(12, 12), holes=True):
    rng = np.random.default_rng(0)
    R = np.cos(np.arange(shape[0])[:, None] / 3.0) * np.sin(np.arange(shape[1])[None, :] / 2.0) + 0.05 * rng.standard_normal(shape)
    if holes:
        R.ravel()[rng.permutation(R.size)[:40]] = np.nan
    return R


def test_python_refusals_need_no_device(ensure_built):
    """The keyword is checked before the engine is asked for a device: every refusal carries its reason."""
    import gpim_amd
    R = _image()
    X, Xf = gpim_amd.utils.get_sparse_grid(R), gpim_amd.utils.get_full_grid(R)
    with pytest.raises(ValueError, match="objective must be 'nll' or 'loo'"):
        gpim_amd.reconstructor(X, R, Xf, objective="elpd")
    with pytest.raises(NotImplementedError, match="objective='loo'.*inducing points"):
        gpim_amd.reconstructor(X, R, Xf, sparse=True, indpoints=20, objective="loo")
    with pytest.raises(NotImplementedError, match="objective='loo'.*single precision"):
        gpim_amd.reconstructor(X, R, Xf, precision="single", objective="loo")
    Rf = _image(holes=False)
    Xg = gpim_amd.utils.get_full_grid(Rf)
    with pytest.raises(NotImplementedError, match="objective='loo'.*Kron solver.*factorise"):
        gpim_amd.reconstructor(Xg, Rf, Xg, structured=True, objective="loo")
    with pytest.raises(NotImplementedError, match="objective='loo'.*Reflection solver.*blocks"):
        gpim_amd.reconstructor(Xg, Rf, Xg, kernel="Matern52", structured=True, objective="loo")
    with pytest.raises(NotImplementedError, match="objective='loo'.*Kron solver"):
        gpim_amd.skreconstructor(Xg, Rf, Xg, objective="loo")
    with pytest.raises(NotImplementedError, match="objective='loo'.*spectral-mixture"):
        gpim_amd.skreconstructor(Xg, Rf, Xg, kernel="Spectral", objective="loo")
    Y = np.stack([Rf, 2.0 * Rf], axis=-1)
    with pytest.raises(NotImplementedError, match="objective='loo'.*multi-output"):
        gpim_amd.vreconstructor(Xg, Y, Xg, objective="loo")
    with pytest.raises(ValueError, match="objective must be"):
        gpim_amd.vreconstructor(Xg, Y, Xg, objective="LOO")


def test_solver_classes_state_their_reason():
    """Kron / Reflection / Columns / SpectralBlocks / Sparse refuse loo_fit and loo_grad with a reason; Dense has none."""
    from gpim_amd import _solvers

    class Owner:
        precision = "double"

    assert _solvers.Dense.no_loo_objective is None
    for cls in (_solvers.Sparse, _solvers.Kron, _solvers.Columns, _solvers.Reflection, _solvers.SpectralBlocks):
        solver = cls.__new__(cls)
        for call in (lambda: solver.loo_fit(Owner(), 0.1, 1, None, None), lambda: solver.loo_grad(Owner(), None)):
            with pytest.raises(NotImplementedError, match="objective='loo': the %s solver" % cls.__name__):
                call()
