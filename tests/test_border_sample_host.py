"""
The identity behind the draws on a grid with missing points, fixed on the CPU in float64: the recipe of
tests/border_sample_oracle.py (A^-1, V and S of the completed grid, explicit) against the dense recipe
pathwise_oracle.draws with idx = the observed points on the same z.

Bar: the project's 10 x pathwise_oracle.HOST_DISCREPANCY x cond, cond the largest among K_GG + s I on the completed grid and
the prior blocks K_b + d I (border_sample_oracle.condition).
"""
import numpy as np
import pytest

import border_sample_oracle as BS
import pathwise_oracle as PO

GRIDS = ((6, 5), (5, 5), (8, 8), (4, 3, 4))
KINDS = ("RBF", "Matern52", "RationalQuadratic")
CASES = tuple((shape, kind, name) for shape in GRIDS for kind in KINDS for name in BS.missing_sets(shape))


def case_id(c):
    return "%s-%s-%s" % ("x".join(str(n) for n in c[0]), c[1], c[2])


def make(shape, kind):
    d = len(shape)
    P = PO.Params(kind, 1.3, [2.0, 3.1, 1.7][:d], 0.02, alpha=1.7, jitter=1e-5)
    blocks = PO.Blocks(PO.full_grid(shape)[0])
    y = np.sin(blocks.G.sum(1) / 5.0) + 0.1 * np.random.default_rng(1).standard_normal(blocks.M)
    return P, blocks, y


def test_missing_sets_cover_the_cases():
    for shape in GRIDS:
        sets = BS.missing_sets(shape)
        assert ("plane" in sets) == any(n % 2 for n in shape)
        rep = PO.Blocks(PO.full_grid(shape)[0]).S["rep"]
        a, b = sets["pair"]
        assert a != b and rep[a] == rep[b]
        assert len(sets["single"]) == 1 and len(set(sets["random"])) == len(sets["random"]) >= 2


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_border_recipe_is_the_dense_recipe(case):
    shape, kind, name = case
    P, blocks, y = make(shape, kind)
    M = blocks.M
    miss = BS.missing_sets(shape)[name]
    bar = 10.0 * PO.HOST_DISCREPANCY * BS.condition(P, blocks)
    for noiseless in (True, False):
        Z = np.random.default_rng(3 + noiseless).standard_normal((3, 2 * M + (0 if noiseless else M)))
        Zp, idx = BS.pathwise_z(Z, M, miss)
        ref = PO.draws(P, blocks, idx, y[idx], Zp, noiseless)
        yn = y.copy()
        yn[miss] = np.nan                   # what lies at the missing points is never read
        got = BS.draws(P, blocks, miss, yn, Z, noiseless)
        err, errm = np.abs(got["out"] - ref["out"]).max(), np.abs(got["mean"] - ref["mean"]).max()
        am = np.abs(got["alpha"][:, miss]).max()
        print("%s noiseless=%d: border - dense %.3e, mean %.3e, |alpha~[m]| %.3e (bar %.3e)"
              % (case_id(case), noiseless, err, errm, am, bar))
        assert err <= bar and errm <= bar
        assert am <= bar
        # entries of z_e at the missing points are ignored; a draw is a function of its own row of z
        Z2 = Z.copy()
        Z2[:, M + miss] = 7.0
        assert np.array_equal(BS.draws(P, blocks, miss, yn, Z2, noiseless)["out"], got["out"])
        one = BS.draws(P, blocks, miss, yn, Z[1:2], noiseless)["out"][0]
        assert np.abs(one - got["out"][1]).max() <= bar


@pytest.mark.parametrize("case", tuple(c for c in CASES if c[1] == "Matern52"), ids=case_id)
def test_embedded_inverse_and_mean(case):
    """E = A^-1 - V S^-1 V^T is (K_oo + s I)^-1 embedded in the grid, and the recipe's mean is the dense posterior mean."""
    shape, kind, name = case
    P, blocks, y = make(shape, kind)
    M = blocks.M
    miss = BS.missing_sets(shape)[name]
    obs = BS.observed(M, miss)
    idx = np.flatnonzero(obs)
    Q = BS.pieces(P, blocks, miss)
    Koo = PO.kmat(P, blocks.G[idx], blocks.G[idx]) + P.s * np.eye(len(idx))
    want = np.zeros((M, M))
    want[np.ix_(idx, idx)] = np.linalg.inv(Koo)
    cond = BS.condition(P, blocks)
    bar = 10.0 * PO.HOST_DISCREPANCY * cond
    err = np.abs(Q["E"] - want).max()
    print("%s: |E - embed(inv(K_oo + s I))| %.3e (bar %.3e)" % (case_id(case), err, bar))
    assert err <= bar
    mean = BS.draws(P, blocks, miss, y, np.zeros((1, 2 * M)), True)["mean"]
    dense = PO.kmat(P, blocks.G, blocks.G[idx]) @ np.linalg.solve(Koo, y[idx])
    assert np.abs(mean - dense).max() <= 10.0 * PO.HOST_DISCREPANCY * cond


def test_oracle_rejects_bad_jitter():
    P, blocks, y = make((5, 5), "RBF")
    for d in (0.0, -1e-6, P.s * 1.01):
        with pytest.raises(ValueError):
            BS.draws(P, blocks, [3], y, np.zeros((1, 2 * blocks.M)), True, d=d)


def test_entry_is_declared_and_bound(ensure_built):
    """include/gpimhip.h declares gpimhip_sample_border and the binding types it (tests/test_cabi_exports.py holds the two
    lists to each other); without a handle the entry refuses before anything touches a device."""
    import ctypes
    import os
    import re
    from gpim_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gpimhip.h")).read(), flags=re.S)
    assert re.search(r"\bgpimhip_sample_border\s*\(", text)
    assert "gpimhip_sample_border" in _lib.EXPORTS
    fn = _lib.load().gpimhip_sample_border
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 19
    assert fn(None, None, None, 0, None, 1, 1, None, None, None, 1, None, None, None, 1, 0, 1e-5, None, None) == _lib.E_BADARG


def test_python_surface_names():
    import gpim_amd
    assert "method='border'" in gpim_amd.reconstructor.sample.__doc__
    assert callable(gpim_amd._solvers.Reflection.sample_border)
    for cls in (gpim_amd._solvers.Dense, gpim_amd._solvers.Sparse, gpim_amd._solvers.Kron):
        with pytest.raises(NotImplementedError):
            cls.sample_border(None, None)
