"""
The identity behind gpimhip_sample_exact, checked on the CPU in float64 (no GPU): in the Cholesky factor of the joint
covariance of the stacked points [X; Xs] the lower-right block IS chol(Sigma) of the posterior covariance, the lower-left
block is W^T = (L^-1 K*)^T, and mean / variance follow from them.  Plus the binding of the new entry point.
"""
import numpy as np
import pytest
import torch
from numpy.testing import assert_allclose

import sample_oracle as SO

# chol(Sigma) is a forward quantity: two float64 routes differ by eps * cond(Sigma) * |L| (measured <= 1.7e-12 on these
# inputs, worst noiseless with overlapping points); the bar of the GPU tests
ATOL = 1e-10


@pytest.mark.parametrize("case", SO.CASES, ids=SO.case_id)
def test_joint_factor_holds_chol_sigma(case):
    R = SO.reference(case)
    N, M, noiseless = case[1], case[2], case[5]
    Lj = SO.joint_factor(R["kp"], R["X"], R["Xs"], SO.JITTER, noiseless, SO.JITTER)
    L22 = Lj[N:, N:]
    assert_allclose(L22.numpy(), R["L"].numpy(), rtol=0, atol=ATOL)
    assert_allclose((L22 @ L22.t()).numpy(), R["Sigma"].numpy(), rtol=0, atol=ATOL)
    # mean = L21 z, var_i = sum_k L22[i,k]^2 - d + noise: the definitions of ExactGP.predict
    z = torch.linalg.solve_triangular(Lj[:N, :N], R["y"].unsqueeze(-1), upper=False).squeeze(-1)
    mean = Lj[N:, :N] @ z
    noise = R["kp"].noise.detach()
    d_s = (0.0 if noiseless else noise) + SO.JITTER
    var = (L22 ** 2).sum(1) - d_s + noise
    m_ref, v_ref = SO.O.ExactGP(R["X"], R["y"], R["kp"], SO.JITTER).predict(R["Xs"])
    assert_allclose(mean.numpy(), m_ref.numpy(), rtol=0, atol=ATOL)
    assert_allclose(mean.numpy(), R["mean"].numpy(), rtol=0, atol=ATOL)
    assert_allclose(var.numpy(), v_ref.numpy(), rtol=0, atol=ATOL)
    assert_allclose(var.numpy(), R["var"].numpy(), rtol=0, atol=ATOL)
    assert M == len(R["Xs"]) and N == len(R["X"])


def test_cases_cover_the_tile_boundaries():
    sizes = {(c[1], c[2]) for c in SO.CASES}
    assert sizes == {(100, 1), (100, 77), (256, 128), (300, 129), (300, 300), (700, 129), (300, 576), (700, 400)}
    assert {c[3] for c in SO.CASES} == {2, 3} and {c[0] for c in SO.CASES} == set(SO.KINDS)
    R = SO.reference(("RBF", 300, 576, 2, "grid", 1))
    # the grid-shaped test points contain every training point
    pts = {tuple(p) for p in R["Xs"].numpy().tolist()}
    assert all(tuple(p) in pts for p in R["X"].numpy().tolist())


def test_binding_has_sample_exact(ensure_built):
    import ctypes
    from gpim_amd import _lib
    assert "gpimhip_sample_exact" in _lib.EXPORTS
    lib = _lib.load()
    fn = lib.gpimhip_sample_exact
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 15
    # no handle: refused before anything touches a device
    assert fn(None, None, None, None, 1, None, None, 1, None, 1, 0, 0.0, None, None, None) == _lib.E_BADARG


def test_python_surface_names():
    import gpim
    import gpim_amd
    from gpim.gpbayes import acqfunc
    assert acqfunc.thompson_sampling is gpim_amd.acqfunc.thompson_sampling
    assert callable(gpim_amd.reconstructor.sample)
    assert "torch.randn((n_samples, M), dtype=torch.float64, device=dev, generator=g)" in gpim_amd.reconstructor.sample.__doc__
