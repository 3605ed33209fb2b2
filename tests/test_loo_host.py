"""
Leave-one-out cross-validation without a GPU: the references of tests/loo_oracle.py against each other, so that the GPU
tests (tests/test_gpu_loo.py) may trust the closed form where N refits are too slow, and the reflection-block assembly --
the arithmetic of loo_finish_kernel's reflection arm, fed by gprutils.reflection_blocks -- against the dense inverse.
"""
import numpy as np
import pytest
import torch
from numpy.testing import assert_allclose

import loo_oracle as LO
from gpim_amd import gprutils


@pytest.mark.parametrize("kind", ["RBF", "Matern52", "RationalQuadratic"])
@pytest.mark.parametrize("N,d,iso", [(40, 2, False), (130, 3, False), (300, 2, True)])
def test_closed_form_equals_refits(kind, N, d, iso):
    kp, _, _, X, y = LO.problem(kind, N, d, iso)
    mb, vb = LO.brute(kp, X, y)
    mc, vc = LO.closed(kp, X, y)
    print("%s N=%d: max |mean| %.2e, max |var| %.2e" % (kind, N, np.abs(mb - mc).max(), np.abs(vb - vc).max()))
    assert_allclose(mc, mb, rtol=0, atol=1e-10)
    assert_allclose(vc, vb, rtol=0, atol=1e-10)


def test_jitter_belongs_to_the_matrix_not_to_the_variance():
    """predict()'s convention: without the `- jitter` term the closed-form variance is off by exactly the jitter"""
    kp, _, _, X, y = LO.problem("Matern52", 40, 2, False)
    _, vb = LO.brute(kp, X, y)
    _, vc = LO.closed(kp, X, y)
    assert np.abs(vc - vb).max() < 1e-10 and np.all(vc - kp.noise.item() > 1e-3)      # (no clamp in play)
    assert_allclose((vc + LO.JITTER) - vb, LO.JITTER, rtol=1e-5)


def test_score():
    rng = np.random.default_rng(0)
    mean, y = rng.standard_normal(50), rng.standard_normal(50)
    var = rng.uniform(0.1, 2.0, 50)
    elpd, sse = LO.score(mean, var, y)
    ref = torch.distributions.Normal(torch.from_numpy(mean), torch.from_numpy(var).sqrt()).log_prob(torch.from_numpy(y)).sum()
    assert_allclose(elpd, ref.item(), rtol=1e-13)
    assert_allclose(sse, ((y - mean) ** 2).sum(), rtol=1e-14)


@pytest.mark.parametrize("kind", ["Matern52", "RationalQuadratic"])
@pytest.mark.parametrize("shape", [(6, 5), (5, 5), (8, 7), (4, 3, 4)])
def test_reflection_assembly_equals_dense_inverse(kind, shape):
    d = len(shape)
    R = LO.smooth_grid(shape, seed=sum(shape))
    Xg = np.array(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"))
    axes = [np.arange(n, dtype=np.float64) for n in shape]
    S = gprutils.reflection_blocks(Xg, R, axes)
    assert S["B"] == 2 ** d and S["sgn"].shape == (R.size,) and S["sgn"].max() == S["B"] - 1
    kp, _, _ = LO.pair(kind, d, [[0.5] * d, [12.0] * d], seed=1)
    X = torch.from_numpy(Xg.reshape(d, -1).T.copy())
    with torch.no_grad():
        K = kp.K(X).numpy().copy()
        K[np.diag_indices(R.size)] += LO.JITTER + kp.noise.item()
    Ki = np.linalg.inv(K)
    dd, alpha = LO.reflection_assembly(S, kp)
    print("%s %s: max |diag| %.2e, max |alpha| %.2e" % (kind, shape, np.abs(dd - np.diag(Ki)).max(),
                                                       np.abs(alpha - Ki @ R.reshape(-1)).max()))
    assert_allclose(dd, np.diag(Ki), rtol=0, atol=1e-11)
    assert_allclose(alpha, Ki @ R.reshape(-1), rtol=0, atol=1e-11)


def test_entries_are_declared_and_typed():
    from gpim_amd import _lib
    for name in ("gpimhip_loo_exact", "gpimhip_loo_exact_batched", "gpimhip_loo_kron"):
        assert name in _lib.EXPORTS
