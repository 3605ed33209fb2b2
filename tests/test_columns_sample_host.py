"""
Host side of the draws of the dense-by-Kronecker blocks, no GPU: ``gprutils.union_rows`` against
numpy's own set operations, the z permutations of ``gprutils.column_sample_maps``, and the oracle of
tests/columns_sample_oracle.py against itself -- the rule restated with a prior factor and eigen-roots must have the
covariance Sigma_post + c_n I + d T (I (x) K_c(u, u)) T^T, or the GPU test would compare against a wrong yardstick.

Bar: 1e-11 on max|A A^T - (Sigma_post + c_n I + extra)|, 20 x the 4.5e-13 measured on these inputs when the identity was
derived (float64 restatements of the same matrix, entries of the order of s2 <= 1.3, solves of condition up to
s2 N / sigma ~ 1e5).  The extra term is positive semi-definite: its smallest eigenvalue >= -1e-12 max|extra|.
"""
import numpy as np
import pytest

import columns_sample_oracle as CO
from columns_oracle import cube
from gpim_amd.gprutils import column_blocks, column_sample_maps, union_rows

BAR = 1e-11


def check_rows(Xs, Xt):
    P, iX, iT = union_rows(Xs, Xt)
    assert P.dtype == np.float64 and iX.dtype == np.int32 and iT.dtype == np.int32
    assert iX.shape == (len(Xs),) and iT.shape == (len(Xt),)
    # sorted lexicographically, no row twice
    order = np.lexsort(P.T[::-1])
    assert np.array_equal(order, np.arange(len(P)))
    assert len(np.unique(P, axis=0)) == len(P)
    assert np.array_equal(P[iX], Xs)                    # a merged row is represented by the training one
    tol = 1e-12 * np.maximum(1.0, np.abs(np.concatenate([Xs, Xt])).max(axis=0))
    assert (np.abs(P[iT] - Xt) <= tol).all()
    assert np.array_equal(np.unique(np.concatenate([iX, iT])), np.arange(len(P)))
    return P, iX, iT


def pixels(n0, n1, keep, seed=0, step=1.0, shift=0.0):
    g = np.array(np.meshgrid(np.arange(0, n0, step) + shift, np.arange(0, n1, step) + shift, indexing="ij")).reshape(2, -1).T
    if keep is None:
        return g
    return g[np.sort(np.random.default_rng(seed).choice(len(g), size=keep, replace=False))]


def test_union_rows_disjoint():
    Xs, Xt = pixels(6, 5, 12), pixels(6, 5, None, shift=0.25)
    P, iX, iT = check_rows(Xs, Xt)
    assert len(P) == len(Xs) + len(Xt)
    assert np.array_equal(P, np.unique(np.concatenate([Xs, Xt]), axis=0))


def test_union_rows_identical():
    Xs = pixels(6, 5, 12)
    P, iX, iT = check_rows(Xs, Xs.copy())
    assert np.array_equal(P, np.unique(Xs, axis=0)) and np.array_equal(iX, iT)
    # the rows come sorted out of pixels(): the maps are the identity
    assert np.array_equal(iX, np.arange(len(Xs)))


def test_union_rows_test_grid_holds_the_training_pixels():
    Xs, Xt = pixels(8, 7, 34, seed=1), pixels(8, 7, None, step=0.5)
    P, iX, iT = check_rows(Xs, Xt)
    assert np.array_equal(P, np.unique(Xt, axis=0)) and len(P) == len(Xt)
    # row search: every training pixel sits where the test grid has it
    for k, x in enumerate(Xs):
        assert np.array_equal(Xt[np.flatnonzero(iT == iX[k])[0]], x)


def test_union_rows_tolerance():
    Xs = pixels(4, 3, None)
    near = Xs.copy()
    near[:, 1] += 1e-13                                 # merges: represented by the training rows
    P, iX, iT = check_rows(Xs, near)
    assert np.array_equal(P, Xs) and np.array_equal(iX, iT)
    apart = Xs.copy()
    apart[:, 0] += 1e-9                                 # does not merge
    P, iX, iT = check_rows(Xs, apart)
    assert len(P) == 2 * len(Xs) and not np.intersect1d(iX, iT).size
    with pytest.raises(ValueError, match="finite"):
        union_rows(Xs, np.full((1, 2), np.nan))
    with pytest.raises(ValueError, match="rows"):
        union_rows(Xs, np.zeros((3, 1)))


# ---- the oracle against itself ----------------------------------------------------------------------------------
def cube_case(shape, frac, seed, finer):
    Xg, X, y = cube(shape, (0, 1), frac, seed=seed)
    C = column_blocks(X, y)
    axes = [np.arange(n, dtype=np.float64) for n in shape]
    if finer:
        axes = [np.arange(0, n - 0.75, 0.5) for n in shape]
    Xt = np.array(np.meshgrid(axes[0], axes[1], indexing="ij")).reshape(2, -1).T
    return C, Xt, axes[2:]


CASES = [("8x7x5", (8, 7, 5), False), ("8x7x5-finer", (8, 7, 5), True), ("6x5x4x3", (6, 5, 4, 3), False)]


@pytest.mark.parametrize("noiseless", (False, True), ids=("noisy", "noiseless"))
@pytest.mark.parametrize("k", (0, 1))
@pytest.mark.parametrize("name,shape,finer", CASES, ids=[c[0] for c in CASES])
def test_rule_has_the_closed_form_covariance(name, shape, finer, k, noiseless):
    C, Xt, axes_t = cube_case(shape, 0.6, 3, finer)     # 40 % of the pixels observed
    s2, ls_r, lc, noise = CO.PARAMS[k]
    A, mean, cov, extra = CO.rule(C["Xs"], C["axes_c"], C["Y"], Xt, axes_t, s2, ls_r, [lc] * len(axes_t), noise,
                                  CO.MODEL_JITTER, CO.D, noiseless)
    M = cov.shape[0]
    Us, U, N, Mw = CO.widths(C["Xs"], C["axes_c"], Xt, axes_t)
    assert A.shape == (M, Us * U + N + M) and Mw == M
    cn = 0.0 if noiseless else noise
    err = np.abs(A @ A.T - (cov + cn * np.eye(M) + extra)).max()
    lo = np.linalg.eigvalsh(0.5 * (extra + extra.T)).min()
    print("%s/%d noiseless=%d: N_s=%d U_s=%d U=%d M=%d  max|A A^T - rule covariance| = %.3e (bar %.0e), max|extra| = %.3e, "
          "min eig(extra) = %.3e" % (name, k, noiseless, len(C["Xs"]), Us, U, M, err, BAR, np.abs(extra).max(), lo))
    assert err <= BAR
    assert lo >= -1e-12 * np.abs(extra).max()
    # without the extra term the identity does NOT hold at this bar: the term is what the prior factor's jitter costs
    assert np.abs(extra).max() > BAR and np.isfinite(mean).all()


def test_z_permutation_round_trip_spectral_axis_first():
    Xg, X, y = cube((5, 12, 12), (1, 2), 0.4, seed=4)
    C = column_blocks(X, y)
    assert C["complete"] == [0] and C["ragged"] == [1, 2]
    tshape = (9, 12, 12)                                # a finer spectral axis on the same pixels
    e_idx, n_idx, o_idx = column_sample_maps(C, tshape)
    Ns, J = C["Y"].shape
    # z_e: the training points in their own row order (grid order, NaN dropped) land on (N_s, J) where Y has them
    y_rows = y.ravel()[~np.isnan(y.ravel())]
    assert np.array_equal(y_rows[e_idx].reshape(Ns, J), C["Y"])
    # z_n: the test grid's C order -> (M_s, M_c) ragged axes first, and the draws back
    M = int(np.prod(tshape))
    zn = np.random.default_rng(0).standard_normal(M)
    lib = zn[n_idx]
    assert np.array_equal(lib.reshape(12, 12, 9), zn.reshape(tshape).transpose(1, 2, 0))
    assert np.array_equal(lib[o_idx], zn)
    assert sorted(e_idx) == list(range(Ns * J)) and sorted(n_idx) == list(range(M))
