"""
The mathematics of the pathwise posterior draws, fixed on the CPU in float64 before any kernel:
the recipe of tests/pathwise_oracle.py applied to the columns of the identity gives the matrix A with p = A z, and
A A^T must be the posterior covariance of the jittered process,

    Sigma_pw = K_GG + d I - (K_GX + d P)(K + s I)^-1 (K_GX + d P)^T.

Bar: both sides are float64 evaluations of the same matrix; the only ill-conditioned step on either side is the solve with
K + s I, so they may differ by a modest multiple of eps * cond(K + s I) * variance.  TOL takes 100 for that multiple (matrix
orders up to 64 here) -- a number fixed by this reasoning, not by what the code gives; the measured figure is printed and
recorded in pathwise_oracle.HOST_DISCREPANCY.  Leaving the d scatter(idx, alpha) term out must break the identity by
more than 100 x TOL: p is uncorrelated with r, so the term's absence adds exactly d^2 P (K + s I)^-1 P^T to the covariance
(4e-10 ... 8e-10 here, d = 1e-5), and what is left is not the Schur complement of anything.
"""
import numpy as np
import pytest

import pathwise_oracle as PO

GRIDS = ((6, 5), (5, 5), (8, 8), (4, 3, 4))
KINDS = ("RBF", "Matern52", "RationalQuadratic")
CASES = tuple((shape, kind) for shape in GRIDS for kind in KINDS)
EPS = np.finfo(np.float64).eps


def case_id(c):
    return "%s-%s" % ("x".join(str(n) for n in c[0]), c[1])


def make(shape, kind, n_train=7, seed=0):
    d = len(shape)
    P = PO.Params(kind, 1.3, [2.0, 3.1, 1.7][:d], np.exp(-3.0), alpha=1.7, jitter=1e-5)
    Xg, _ = PO.full_grid(shape)
    blocks = PO.Blocks(Xg)
    idx = np.sort(np.random.default_rng(seed).permutation(blocks.M)[:n_train]).astype(np.int64)
    return P, blocks, idx


def tol(P, blocks, idx):
    X = blocks.G[idx]
    return 100.0 * EPS * np.linalg.cond(PO.kmat(P, X, X) + P.s * np.eye(len(idx))) * P.var


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_covariance_identity(case):
    P, blocks, idx = make(*case)
    A = PO.probe_matrix(P, blocks, idx)
    Spw = PO.sigma_pathwise(P, blocks, idx)
    err = np.abs(A @ A.T - Spw).max()
    t = tol(P, blocks, idx)
    # without the scatter term the covariance is not a Schur complement of anything
    A0 = PO.probe_matrix(P, blocks, idx, scatter=False)
    err0 = np.abs(A0 @ A0.T - Spw).max()
    shift = np.abs(Spw - PO.sigma_joint(P, blocks, idx)).max() / P.jitter
    print("A A^T - Sigma_pw %.3e (bar %.3e); without the scatter term %.3e; max|Sigma_pw - Sigma| / d %.4f"
          % (err, t, err0, shift))
    assert err <= t
    assert err0 > 100.0 * t
    # the figures the GPU tests scale (recorded in the oracle module) bound what is measured here
    # (rounding differs between BLAS builds: the recorded discrepancy is held to a factor of two)
    assert err <= 2.0 * PO.HOST_DISCREPANCY
    assert shift <= PO.COV_SHIFT_OVER_D
    # the closed form of the difference to the joint route's covariance
    X = blocks.G[idx]
    Ai = np.linalg.inv(PO.kmat(P, X, X) + P.s * np.eye(len(idx)))
    Pm = np.zeros((blocks.M, len(idx)))
    Pm[idx, np.arange(len(idx))] = 1.0
    Kgx = PO.kmat(P, blocks.G, X)
    d = P.jitter
    diff = -d * (Pm @ Ai @ Kgx.T + Kgx @ Ai @ Pm.T) - d * d * Pm @ Ai @ Pm.T
    assert np.abs((Spw - PO.sigma_joint(P, blocks, idx)) - diff).max() <= t


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_basis_change(case):
    """U from the oracle is the basis change of gprutils.reflection_blocks, orthogonal, and block-diagonalises K_GG into
    the blocks the prior draw factors."""
    from gpim_amd import gprutils
    P, blocks, _ = make(*case)
    U = blocks.U2()
    rows = blocks.present.reshape(-1)
    Up = U[rows]
    assert Up.shape == (blocks.M, blocks.M) and not U[~rows].any()
    assert np.abs(Up @ Up.T - np.eye(blocks.M)).max() <= 8 * EPS
    # reflection_blocks' forward direction on a random y
    Xg, _ = PO.full_grid(case[0])
    y = np.random.default_rng(5).standard_normal(case[0])
    axes, _ = gprutils.grid_axes(Xg)
    ys = gprutils.reflection_blocks(Xg, y, axes)["ys"]
    assert np.abs((U @ y.reshape(-1)).reshape(ys.shape) - ys).max() <= 16 * EPS * np.abs(y).max()
    # U K_GG U^T = blockdiag(K_b): the blocks by their sum over the mirror images, rows of absent points removed
    K = PO.kmat(P, blocks.G, blocks.G)
    T = U @ K @ U.T
    D = np.zeros_like(T)
    for b, Kb in enumerate(blocks.prior_blocks(P, 0.0)):
        pr = blocks.present[b]
        Kb = Kb.copy()
        Kb[~pr, ~pr] = 0.0                                  # (the identity rows belong to the padding, not to K)
        D[b * blocks.Nq:(b + 1) * blocks.Nq, b * blocks.Nq:(b + 1) * blocks.Nq] = Kb
    assert np.abs(T - D).max() <= 64 * blocks.M * EPS * P.var


def test_prior_draw_covariance():
    """g = U^T blockdiag(chol(K_b + d I)) z has covariance K_GG + d I; z_p reaches every existing row exactly once."""
    P, blocks, _ = make((6, 5), "Matern52")
    src = blocks.zsrc[blocks.present]
    assert sorted(src.tolist()) == list(range(blocks.M))
    Gm = blocks.prior_draw(P, P.jitter, np.eye(blocks.M)).T          # g = Gm z
    K = PO.kmat(P, blocks.G, blocks.G) + P.jitter * np.eye(blocks.M)
    assert np.abs(Gm @ Gm.T - K).max() <= 64 * blocks.M * EPS * P.var


def test_oracle_rejects_bad_jitter():
    P, blocks, idx = make((5, 5), "RBF")
    for d in (0.0, -1e-6, P.s * 1.01):
        with pytest.raises(ValueError):
            PO.draws(P, blocks, idx, np.zeros(len(idx)), np.zeros((1, blocks.M + len(idx))), True, d=d)


def test_pathwise_grid_helper():
    from gpim_amd import gprutils
    Xg, rows = PO.full_grid((6, 5))
    idx = np.array([0, 7, 29, 13])
    G = gprutils.pathwise_grid(Xg, rows[idx])
    assert G["mask"] == 3 and G["shape"] == (6, 5) and G["twoc"][:2] == [5.0, 4.0] and G["idx"].tolist() == idx.tolist()
    with pytest.raises(NotImplementedError, match="not on it"):
        gprutils.pathwise_grid(Xg, rows[idx] + np.array([0.0, 0.5]))
    with pytest.raises(NotImplementedError, match="same grid point"):
        gprutils.pathwise_grid(Xg, rows[[3, 3]])
    skew = Xg.copy()
    skew[0, 2, 3] += 0.25
    with pytest.raises(NotImplementedError, match="product grid"):
        gprutils.pathwise_grid(skew, rows[idx])
    with pytest.raises(NotImplementedError, match="product grid"):
        gprutils.pathwise_grid(rows.T, rows[idx])
    # no symmetric axis: unevenly spaced coordinates along both axes
    ax = [np.array([0.0, 1.0, 3.0, 7.0]), np.array([0.0, 2.0, 3.0])]
    Xu = np.array(np.meshgrid(*ax, indexing="ij"))
    with pytest.raises(NotImplementedError, match="symmetric"):
        gprutils.pathwise_grid(Xu, Xu.reshape(2, -1).T[:3])


def test_binding_has_sample_pathwise(ensure_built):
    import ctypes
    from gpim_amd import _lib
    assert "gpimhip_sample_pathwise" in _lib.EXPORTS
    fn = _lib.load().gpimhip_sample_pathwise
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 16
    # no handle: refused before anything touches a device
    assert fn(None, None, None, None, 1, None, None, None, 1, None, None, 1, 0, 1e-5, None, None) == _lib.E_BADARG


def test_python_surface_names():
    import inspect
    import gpim_amd
    assert inspect.signature(gpim_amd.reconstructor.sample).parameters["method"].default == "joint"
    assert "method='pathwise'" in gpim_amd.reconstructor.sample.__doc__
    assert callable(gpim_amd._solvers.Dense.sample_pathwise)
    assert inspect.signature(gpim_amd.acqfunc.thompson_on_device).parameters["method"].default == "joint"
