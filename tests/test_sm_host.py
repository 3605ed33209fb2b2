"""CPU checks of the spectral-mixture kernel of skreconstructor(kernel='Spectral') (no GPU): the engine's closed-form
gradient against the dense restatement's autograd, the initialisation against an independent restatement, and the C ABI
names of the new entry points."""
import ctypes

import numpy as np
import pytest

import sm_oracle as S

SM_SYMBOLS = ("gpimhip_sm_kmat", "gpimhip_sm_nll_grad", "gpimhip_fit_sm", "gpimhip_predict_sm")


@pytest.mark.parametrize("isotropic", [False, True])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_closed_form_gradient_equals_autograd(d, isotropic):
    Q = 3
    D = 1 if isotropic else d
    X, y = S.random_data(30, d, seed=d)
    for seed in (1, 2):
        u = S.random_u(Q, D, seed=10 * d + seed)
        _, g0 = S.loss_grad(u, X, y, Q, D)
        g1 = S.closed_grad(u, X, y, Q, D)
        assert np.abs(g1 - g0).max() <= 1e-12 * np.abs(g0).max()
        assert np.all(np.abs(g1 - g0) <= 1e-12 * np.maximum(np.abs(g0), np.abs(g0).max() * 1e-3) + 1e-15)


def _grid_with_holes():
    import gpim_amd
    R = np.sin(np.arange(12)[:, None] / 2.0) * np.cos(np.arange(9)[None, :] / 3.0)
    R[2:5, 3:7] = np.nan
    R[::4, ::3] = np.nan
    X = gpim_amd.utils.get_sparse_grid(R)
    Xt, yt = gpim_amd.utils.prepare_training_data(X, R)
    return Xt.numpy(), yt.numpy()


@pytest.mark.parametrize("isotropic", [False, True])
@pytest.mark.parametrize("Q", [1, 4, 7])
def test_initial_raw_matches_oracle_bitwise(Q, isotropic):
    from gpim_amd.smgpr import initial_raw
    X, y = _grid_with_holes()
    for seed in (0, 3):
        u0 = initial_raw(X, y, Q, isotropic, seed)
        u1 = S.initial_raw(X, y, Q, isotropic, seed)
        assert u0.shape == u1.shape == (2 + Q * (2 * (1 if isotropic else 2) + 1),)
        assert np.array_equal(u0, u1)


def test_initial_raw_scattered_points():
    from gpim_amd.smgpr import initial_raw
    X, y = S.random_data(50, 3, seed=7)
    assert np.array_equal(initial_raw(X, y, 4, False, 5), S.initial_raw(X, y, 4, False, 5))


def test_constrained_map_matches_oracle():
    from gpim_amd.smgpr import constrained
    Q, D = 3, 2
    u = S.random_u(Q, D, seed=4)
    c, w, m, s, noise = constrained(u, Q, D)
    row = S.constrained_row(u, Q, D)
    assert np.allclose(np.concatenate([[c], w, m.ravel(), s.ravel(), [noise]]), row, rtol=1e-15, atol=0)


def test_sm_entry_points_exported_and_bound(ensure_built):
    from gpim_amd import _lib
    lib = ctypes.CDLL(ensure_built)
    for name in SM_SYMBOLS:
        assert hasattr(lib, name)
        assert name in _lib.EXPORTS
    assert ctypes.sizeof(_lib.SmStruct) == 16
    assert _lib.SM_MAX_MIXTURES == 16


def test_spectral_dispatch_without_gpu_fails_loudly():
    """Without a GPU the Spectral branch exists and raises the engine's RuntimeError (not KeyError / TypeError)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import gpim
    R = np.random.rand(8, 8)
    R[::2, ::2] = np.nan
    X = gpim.utils.get_sparse_grid(R)
    with pytest.raises(RuntimeError):
        gpim.skreconstructor(X, R, gpim.utils.get_full_grid(R), 'Spectral', sparse=True, grid_points_ratio=1.)
