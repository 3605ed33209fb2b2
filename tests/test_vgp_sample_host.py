"""
The identity behind vreconstructor.sample, on the host in float64: the block reduction of the
multi-output GP diagonalises the posterior, so T single-output draws of the latent blocks, mixed back, have exactly the dense
N T model's posterior mean and covariance.  tests/vgp_sample_oracle.py holds both sides; the GPU tests reuse them.

Bar: 1e-11 absolute on mean, variance and every entry of the covariance (the rounding of the two float64 routes; the figures
reached are printed with -s).
"""
import numpy as np
import pytest

import pathwise_oracle as PO
import vgp_oracle as VO
import vgp_sample_oracle as VS

ATOL = 1e-11
JITTER = 1e-5


strong_u = VS.strong_u


# (T, N, M, kernel, test points on the training points, noiseless, independent, identical tasks)
CASES = ((3, 150, 90, "RBF", False, False, False, False),
         (3, 150, 90, "RBF", True, True, False, False),
         (2, 200, 100, "RBF", True, True, False, False),
         (4, 130, 130, "RBF", True, False, False, False),
         (3, 120, 70, "RBF", False, False, True, False),
         (3, 120, 70, "RBF", True, True, False, True),
         (3, 150, 90, "Matern52", True, True, False, False),
         (1, 130, 60, "RBF", False, False, False, False))


def case_id(c):
    return "T%d-N%d-M%d-%s-%s-%s%s%s" % (c[0], c[1], c[2], c[3], "on" if c[4] else "off", "noiseless" if c[5] else "noisy",
                                         "-independent" if c[6] else "", "-identical" if c[7] else "")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_mixed_block_draws_have_the_dense_posterior(case):
    T, N, M, kernel, on, noiseless, independent, identical = case
    X, Y = VO.random_data(N, T, 2, seed=N + T)
    Xs = X[:M].copy() if on else np.random.default_rng(N).uniform(0.0, 8.0, size=(M, 2))
    u = strong_u(T, 2, independent, seed=T + M, identical=identical)
    mean_d, Sig = VS.dense(u, X, Y, Xs, kernel, independent, None, noiseless, JITTER)
    s = VS.params(u, T, 2, independent, None)[2]
    for eig in ("eigh", "jacobi"):
        R = VS.Recipe(u, X, Y, kernel, independent, None, eig=eig)
        J = R.joint(Xs, noiseless, JITTER)
        A = R.joint_factor(J)
        e_cov = np.abs(A @ A.T - Sig).max()
        e_mean = np.abs(J["mean"] - mean_d).max()
        # the variance of predict: noise included, jitter excluded
        var_d = np.diag(Sig).reshape(M, T) - JITTER * s + (s if noiseless else 0.0)
        e_var = np.abs(J["var"] - var_d).max()
        print("%s %s: lambda max %.1f, cond Sigma %.2e, |D D^T - Sigma| %.2e, mean %.2e, var %.2e"
              % (case_id(case), eig, R.lam.max(), PO.cond_spd(Sig), e_cov, e_mean, e_var))
        assert e_cov <= ATOL and e_mean <= ATOL and e_var <= ATOL
        # a draw is mean + A z
        Z = np.random.default_rng(1).standard_normal((T, 3, M))
        got = R.joint_draws(J, Z)
        want = J["mean"][None] + (Z.reshape(T, 3, M).transpose(1, 0, 2).reshape(3, T * M) @ A.T).reshape(3, M, T)
        assert np.abs(got - want).max() <= ATOL
    if identical:
        lam = np.sort(R.lam)
        assert np.abs(lam[:-1] - lam[0]).max() <= 1e-12 * lam[-1]          # the repeated eigenvalue is there
    # the oracle's Jacobi iteration is an eigen-decomposition
    lam_j, Q = VS.jacobi(R.B / np.sqrt(np.outer(R.s, R.s)))
    assert np.abs(Q @ np.diag(lam_j) @ Q.T - R.B / np.sqrt(np.outer(R.s, R.s))).max() <= 1e-13 * max(1.0, lam_j.max())
    assert np.abs(Q.T @ Q - np.eye(T)).max() <= 1e-14


# 8x7: one symmetric axis would do, both are; 6x6: two; 5x4x4: a cube with mirror planes (odd axis)
GRIDS = (((8, 7), 3, "RBF"), ((6, 6), 2, "Matern52"), ((5, 4, 4), 2, "RBF"))


def grid_problem(shape, T, seed=0):
    Xg, G = PO.full_grid(shape)
    rng = np.random.default_rng(seed + len(G))
    base = np.stack([np.sin(G @ rng.normal(size=len(shape)) * 0.5 + rng.uniform(0, 6)) for _ in range(3)], 1)
    Y = base @ rng.normal(size=(3, T)) + 0.1 * rng.normal(size=(len(G), T)) + rng.normal(size=T)
    return Xg, G, Y


def unit_probes(T, W):
    """Z (T, T W, W): draw t W + k has the unit vector e_k in block t and zeros elsewhere."""
    Z = np.zeros((T, T * W, W))
    for t in range(T):
        Z[t, t * W:(t + 1) * W] = np.eye(W)
    return Z


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(str(n) for n in g[0]))
def test_mixed_block_draws_on_a_full_grid(grid):
    shape, T, kernel = grid
    d = len(shape)
    Xg, G, Y = grid_problem(shape, T)
    M = len(G)
    blocks = PO.Blocks(Xg)
    u = strong_u(T, d, False, seed=M)
    R = VS.Recipe(u, G, Y, kernel, False, None, eig="jacobi")
    for noiseless in (True, False):
        mean_d, Sig = VS.dense_blocks(u, G, Y, kernel, False, None, noiseless, JITTER)
        W = 2 * M + (0 if noiseless else M)
        out = R.blocks_draws(blocks, unit_probes(T, W), noiseless, JITTER)
        A = (out["out"] - out["mean"][None]).reshape(T * W, M * T).T
        e_cov, e_mean = np.abs(A @ A.T - Sig).max(), np.abs(out["mean"] - mean_d).max()
        print("%s T=%d %s noiseless=%d: lambda max %.1f, |A A^T - Sigma| %.2e, mean %.2e"
              % ("x".join(map(str, shape)), T, kernel, noiseless, R.lam.max(), e_cov, e_mean))
        assert e_cov <= ATOL and e_mean <= ATOL
