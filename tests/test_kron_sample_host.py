"""
Host side of the Kronecker posterior draws, no GPU: ``gprutils.union_axes`` against numpy's own
set operations, and the oracle of tests/kron_sample_oracle.py against itself -- the rule restated with eigh must have the
covariance that the dense Cholesky posterior has, A A^T = Sigma_post + c I, or the GPU test would compare against a wrong
yardstick.

Bar: 1e-12 on max|A A^T - (Sigma_post + c I)|.  Both sides are float64 restatements of the same matrix with entries of the
order of s2 <= 9 and condition numbers up to s2 N / sigma ~ 1e6 in the solves; their rounding is eps x that x a few, and the
worst case measured when the construction was written was 3.7e-14.
"""
import numpy as np
import pytest

import kron_sample_oracle as KO
from gpim_amd.gprutils import union_axes

BAR = 1e-12


def check_union(c, t):
    au, ic, it = union_axes(c, t)
    assert len(au) == len(ic) == len(it) == len(c)
    for i in range(len(c)):
        assert au[i].dtype == np.float64 and ic[i].dtype == np.int32 and it[i].dtype == np.int32
        assert np.all(np.diff(au[i]) > 0)
        assert ic[i].shape == np.shape(c[i]) and it[i].shape == np.shape(t[i])
        assert np.array_equal(au[i][ic[i]], c[i])
        assert np.allclose(au[i][it[i]], t[i], rtol=0, atol=1e-12 * max(1.0, np.abs(au[i]).max()))
    return au, ic, it


def test_union_identical_axes_give_identity():
    c = [np.arange(6.0), np.linspace(-2, 2, 5)]
    au, ic, it = check_union(c, [a.copy() for a in c])
    for i in range(2):
        assert np.array_equal(au[i], c[i])
        assert np.array_equal(ic[i], np.arange(len(c[i]))) and np.array_equal(it[i], np.arange(len(c[i])))


def test_union_finer_grid():
    c, t = [np.arange(6.0), np.arange(5.0)], [np.arange(0, 5.5, .5), np.arange(0, 4.5, .5)]
    au, ic, it = check_union(c, t)
    for i in range(2):
        ref = np.unique(np.concatenate([c[i], t[i]]))
        assert np.array_equal(au[i], ref)
        assert np.array_equal(ic[i], np.searchsorted(ref, c[i])) and np.array_equal(it[i], np.searchsorted(ref, t[i]))
        assert np.array_equal(ic[i], 2 * np.arange(len(c[i])))


def test_union_shifted_grid_merges_nothing():
    c, t = [np.arange(6.0)], [np.arange(6.0) + 0.37]
    au, ic, it = check_union(c, t)
    ref = np.unique(np.concatenate([c[0], t[0]]))
    assert len(au[0]) == 12 and np.array_equal(au[0], ref)
    assert np.array_equal(ic[0], np.searchsorted(ref, c[0])) and np.array_equal(it[0], np.searchsorted(ref, t[0]))


def test_union_crop_leaves_the_training_axis():
    c, t = [np.arange(6.0), np.arange(5.0)], [np.array([1., 2., 3.]), np.array([2., 3., 4.])]
    au, ic, it = check_union(c, t)
    for i in range(2):
        assert np.array_equal(au[i], c[i]) and np.array_equal(ic[i], np.arange(len(c[i])))
        assert np.array_equal(it[i], np.searchsorted(c[i], t[i]))


def test_union_merges_coordinates_1e14_apart():
    c, t = [np.array([0.0, 1.0, 2.0])], [np.array([0.5, 1.0 + 1e-14, 2.0 - 1e-14, 3.0])]
    au, ic, it = check_union(c, t)
    assert np.array_equal(au[0], [0.0, 0.5, 1.0, 2.0, 3.0])          # the training coordinate stands for the pair
    assert np.array_equal(ic[0], [0, 2, 3]) and np.array_equal(it[0], [1, 2, 3, 4])
    # the tolerance scales with the coordinates: 1e-9 apart merges at 1e4, not at 1
    assert len(union_axes([np.array([1e4])], [np.array([1e4 + 1e-9])])[0][0]) == 1
    assert len(union_axes([np.array([1.0])], [np.array([1.0 + 1e-9])])[0][0]) == 2


def test_union_axis_of_length_one():
    au, ic, it = check_union([np.array([3.0]), np.arange(4.0)], [np.array([3.0]), np.array([1.5])])
    assert np.array_equal(au[0], [3.0]) and np.array_equal(ic[0], [0]) and np.array_equal(it[0], [0])
    assert np.array_equal(au[1], [0, 1, 1.5, 2, 3]) and np.array_equal(it[1], [2])


def test_union_refuses_what_it_cannot_take():
    with pytest.raises(ValueError):
        union_axes([np.arange(3.0)], [np.arange(3.0), np.arange(2.0)])
    with pytest.raises(ValueError):
        union_axes([np.arange(3.0)], [np.array([0.0, np.nan])])


@pytest.mark.parametrize("noiseless", (False, True))
@pytest.mark.parametrize("name,k", KO.CASES, ids=lambda v: str(v))
def test_oracle_rule_has_the_posterior_covariance(name, k, noiseless):
    c, t, ls, s2, noise = KO.case(name, k)
    _, cov = KO.posterior(c, t, ls, s2, noise, KO.MODEL_JITTER)
    A = KO.draw_matrix(c, t, ls, s2, noise, KO.MODEL_JITTER, noiseless, KO.MODEL_JITTER)
    PU, N, M = KO.widths(c, t)
    assert A.shape == (M, PU + N + M)
    cc = (0.0 if noiseless else noise) + KO.MODEL_JITTER
    err = np.abs(A @ A.T - (cov + cc * np.eye(M))).max()
    print("%s/%d noiseless=%d: max|A A^T - (Sigma_post + c I)| = %.3e (bar %.1e)" % (name, k, noiseless, err, BAR))
    assert err <= BAR


def test_oracle_mean_is_the_rule_at_zero():
    """the mean the rule gives at z = 0, s2 Ks_ Q D^-1 Q^T y, is the Cholesky posterior's"""
    c, t, ls, s2, noise = KO.case("shifted", 0)
    y = np.sin(KO.points(c).sum(1) / 3.0)
    mean, _ = KO.posterior(c, t, ls, s2, noise, KO.MODEL_JITTER, y)
    A = KO.draw_matrix(c, t, ls, s2, noise, KO.MODEL_JITTER, True, 0.0)
    PU, N, M = KO.widths(c, t)
    G = -A[:, PU:PU + N] / np.sqrt(noise + KO.MODEL_JITTER)
    assert np.abs(G @ y - mean).max() <= 1e-12
    assert not A[:, PU + N:].any()
