"""
Reference for the joint posterior draws (gpimhip_sample_exact), float64 on the CPU with the oracle's kernels
(oracle/gpim_oracle.py), by the explicit route of ExactGP.predict:

    W = L^-1 K*  (solve_triangular),   mean = W^T L^-1 y,   Sigma = K** - W^T W + d I,   d = (noiseless ? 0 : noise) + jitter_s

and, independently, the Cholesky factor of the joint covariance of [X; Xs] whose lower-right block is chol(Sigma) -- the
identity the engine is built on.  Every diagonal term is added as float64.  Shared by tests/test_sample_host.py and
tests/test_gpu_sample.py: the inputs, the cases and the cached references live here.
"""
import functools

import numpy as np
import torch

from oracle import gpim_oracle as O

_F64 = torch.float64
JITTER = 1e-5
KINDS = ("RBF", "Matern52", "RationalQuadratic")
# (N, M, d, test points): the K / K* boundary of the stacked points on a tile edge (256), inside a 128-tile (100, 300, 700),
# M = 1, both parts below one tile, a nearly empty last tile (300 + 129 = 3 x 128 + 45 -> 429), M > N, a grid-shaped
# Xs that contains every training point (24 x 24 = 576), and one order above 1024
SIZES = ((100, 1, 2, "random"), (100, 77, 3, "random"), (256, 128, 2, "random"), (300, 129, 3, "random"),
         (300, 300, 2, "overlap"), (700, 129, 3, "random"), (300, 576, 2, "grid"),
         # order 1100 -> 1152: from order 1024 on the joint matrix has padded rows (row stride order + 16)
         (700, 400, 3, "random"))
CASES = tuple((kind, N, M, d, how, noiseless) for (N, M, d, how) in SIZES for kind in KINDS for noiseless in (0, 1))


def case_id(c):
    return "%s-N%d-M%d-d%d-%s-%s" % (c[0], c[1], c[2], c[3], c[4], "noiseless" if c[5] else "noisy")


def scattered(N, d, seed, grid=24):
    """the scattered points of tests/test_gpu_ops.py"""
    rng = np.random.default_rng(seed)
    X = np.unique(rng.integers(0, grid, size=(N * 4, d)), axis=0).astype(np.float64)
    rng.shuffle(X)
    X = X[:N]
    y = np.sin(X.sum(1) / 5.0) + 0.1 * rng.standard_normal(len(X))
    return torch.from_numpy(np.ascontiguousarray(X)), torch.from_numpy(y)


def pair(kind, d, ls, seed, jitter=JITTER, noise_u=-3.0):
    """(oracle KernelParams, gpim_amd KernelSpec, u) holding identical parameters (as tests/test_gpu_ops.py)."""
    from gpim_amd.kernels import KernelSpec
    torch.manual_seed(seed)
    kp = O.KernelParams(kind, d, ls)
    torch.manual_seed(seed)
    spec = KernelSpec(kind, d, ls, jitter=jitter)
    u = spec.draw_initial_u()
    with torch.no_grad():
        kp.u_noise.fill_(noise_u)
    u[1 + spec.n_ls] = noise_u
    return kp, spec, u


def test_points(X, M, d, how, seed=11):
    if how == "grid":
        assert d == 2 and M == 576
        ii, jj = np.meshgrid(np.arange(24.0), np.arange(24.0), indexing="ij")
        return torch.from_numpy(np.stack([ii.ravel(), jj.ravel()], axis=1))
    Xs = torch.from_numpy(np.random.default_rng(seed).uniform(0, 24, size=(M, d)))
    if how == "overlap":                      # every third test point is a training point
        Xs[::3] = X[:len(Xs[::3])]
    return Xs


def _with_diag(K, add):
    K = K.contiguous().clone()
    n = K.shape[0]
    K.view(-1)[::n + 1] += torch.as_tensor(add, dtype=_F64)
    return K


@torch.no_grad()
def explicit(kp, X, y, Xs, jitter, noiseless, jitter_s):
    """(mean, Sigma, chol Sigma, var) by the route of ExactGP.predict; var = diag(Sigma) - d + noise."""
    noise = kp.noise.detach().to(_F64)
    d_s = (torch.zeros((), dtype=_F64) if noiseless else noise) + torch.as_tensor(jitter_s, dtype=_F64)
    L = torch.linalg.cholesky(_with_diag(kp.K(X), torch.as_tensor(jitter, dtype=_F64) + noise))
    pack = torch.cat((y.unsqueeze(-1), kp.K(X, Xs)), dim=1)
    Sv = torch.linalg.solve_triangular(L, pack, upper=False)
    W = Sv[:, 1:]
    mean = W.t().matmul(Sv[:, :1]).squeeze(-1)
    Sigma = _with_diag(kp.K(Xs) - W.t().matmul(W), d_s)
    Sigma = 0.5 * (Sigma + Sigma.t())
    var = Sigma.diagonal() - d_s + noise
    return mean, Sigma, torch.linalg.cholesky(Sigma), var


@torch.no_grad()
def joint_factor(kp, X, Xs, jitter, noiseless, jitter_s):
    """chol of the joint covariance of [X; Xs] with the two diagonal terms on their segments."""
    N, M = len(X), len(Xs)
    noise = kp.noise.detach().to(_F64)
    d_s = (torch.zeros((), dtype=_F64) if noiseless else noise) + torch.as_tensor(jitter_s, dtype=_F64)
    add = torch.cat([(torch.as_tensor(jitter, dtype=_F64) + noise).expand(N), d_s.expand(M)])
    J = kp.K(torch.cat([X, Xs]))
    J = 0.5 * (J + J.t())
    J.view(-1)[::N + M + 1] += add
    return torch.linalg.cholesky(J)


@functools.lru_cache(maxsize=None)
def reference(case):
    """Inputs and the explicit reference of one case, computed once: dict with kp, spec, u, X, y, Xs, mean, Sigma, L, var."""
    kind, N, M, d, how, noiseless = case
    X, y = scattered(N, d, seed=N)
    assert len(X) == N
    kp, spec, u = pair(kind, d, [[1.0] * d, [6.0] * d], seed=3)
    Xs = test_points(X, M, d, how)
    mean, Sigma, L, var = explicit(kp, X, y, Xs, JITTER, noiseless, JITTER)
    return dict(kp=kp, spec=spec, u=u, X=X, y=y, Xs=Xs, mean=mean, Sigma=Sigma, L=L, var=var)
