"""
The identity behind the draws on a fully observed grid, fixed on the CPU in float64: the block recipe
of tests/blocks_oracle.py against the dense recipe pathwise_oracle.draws(..., idx=arange(M)) on the same z.

Bar: both are float64 evaluations of the same numbers through Cholesky factors of the same matrices in two bases, so they
differ by the rounding level of the recipe (pathwise_oracle.HOST_DISCREPANCY) times the condition number reported for the
case, with the margin of 10 that tests/test_gpu_pathwise.py gives a different summation order.
"""
import numpy as np
import pytest

import blocks_oracle as BO
import pathwise_oracle as PO

GRIDS = ((6, 5), (5, 5), (8, 8), (4, 3, 4), (16, 16))
KINDS = ("RBF", "Matern52", "RationalQuadratic")
CASES = tuple((shape, kind) for shape in GRIDS for kind in KINDS)
EPS = np.finfo(np.float64).eps


def case_id(c):
    return "%s-%s" % ("x".join(str(n) for n in c[0]), c[1])


def make(shape, kind):
    d = len(shape)
    P = PO.Params(kind, 1.3, [2.0, 3.1, 1.7][:d], 0.02, alpha=1.7, jitter=1e-5)
    blocks = PO.Blocks(PO.full_grid(shape)[0])
    y = np.sin(blocks.G.sum(1) / 5.0) + 0.1 * np.random.default_rng(1).standard_normal(blocks.M)
    return P, blocks, y


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_block_recipe_is_the_dense_recipe(case):
    P, blocks, y = make(*case)
    M = blocks.M
    idx = np.arange(M)
    bar = 10.0 * PO.HOST_DISCREPANCY * PO.condition(P, blocks, idx)
    for noiseless in (True, False):
        Z = np.random.default_rng(3 + noiseless).standard_normal((3, 2 * M + (0 if noiseless else M)))
        ref = PO.draws(P, blocks, idx, y, Z, noiseless)
        got = BO.draws(P, blocks, y, Z, noiseless)
        err, errm = np.abs(got["out"] - ref["out"]).max(), np.abs(got["mean"] - ref["mean"]).max()
        print("%s noiseless=%d: blocks - dense %.3e, mean %.3e (bar %.3e)" % (case_id(case), noiseless, err, errm, bar))
        assert err <= bar and errm <= bar
        # a draw is a function of its own row of z
        one = BO.draws(P, blocks, y, Z[1:2], noiseless)["out"][0]
        assert np.abs(one - got["out"][1]).max() <= bar


@pytest.mark.parametrize("shape", GRIDS, ids=lambda s: "x".join(str(n) for n in s))
def test_forward_basis_change(shape):
    """U U^T = I on the rows that exist, zero rows elsewhere, and U^T (U v) = v: the forward direction inverts the transposed
    one that the prior draw uses."""
    blocks = PO.Blocks(PO.full_grid(shape)[0])
    U = blocks.U2()
    rows = blocks.present.reshape(-1)
    assert rows.sum() == blocks.M and not U[~rows].any()
    assert np.abs(U[rows] @ U[rows].T - np.eye(blocks.M)).max() <= 8 * EPS
    v = np.random.default_rng(2).standard_normal((2, blocks.M))
    f = BO.forward(blocks, v)
    assert f.shape == (2, blocks.B, blocks.Nq) and not f[:, ~blocks.present].any()
    assert np.abs(f.reshape(2, -1) @ U - v).max() <= 16 * EPS * np.abs(v).max()


def test_oracle_rejects_bad_jitter():
    P, blocks, y = make((5, 5), "RBF")
    for d in (0.0, -1e-6, P.s * 1.01):
        with pytest.raises(ValueError):
            BO.draws(P, blocks, y, np.zeros((1, 2 * blocks.M)), True, d=d)


def test_binding_has_sample_blocks(ensure_built):
    import ctypes
    from gpim_amd import _lib
    assert "gpimhip_sample_blocks" in _lib.EXPORTS
    fn = _lib.load().gpimhip_sample_blocks
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 14
    # no handle: refused before anything touches a device
    assert fn(None, None, None, None, 1, None, None, None, None, 1, 0, 1e-5, None, None) == _lib.E_BADARG


def test_python_surface_names():
    import inspect
    import gpim_amd
    assert inspect.signature(gpim_amd.reconstructor.sample).parameters["method"].default == "joint"
    assert "method='blocks'" in gpim_amd.reconstructor.sample.__doc__
    assert callable(gpim_amd._solvers.Dense.sample_blocks)
    assert gpim_amd._solvers.Kron.sample_blocks is gpim_amd._solvers.Dense.sample_blocks
    assert gpim_amd._solvers.Reflection.sample_blocks is gpim_amd._solvers.Dense.sample_blocks
