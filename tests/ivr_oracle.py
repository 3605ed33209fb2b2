"""
CPU references for integrated variance reduction (reconstructor.ivr, gpimhip_ivr_exact), float64 throughout.  With
S = K + (noise + jitter) I, W = L^-1 K(X, G) and C = K(G, G) - W^T W, the latent posterior covariance on the rows G:

  closed(kp, X, G, w, jitter)   the formula the engine uses, in numpy:  a_j = sum_m w_m C_mj^2 / (max(C_jj, 0) + noise + jitter)
  brute(kp, X, G, w, jitter)    the definition: M refits of the dense oracle with candidate j appended,
                                a_j = sum_m w_m (var_before(m) - var_after_adding_j(m))     (y does not enter a variance: zeros)
  latent_var(kp, X, G, jitter)  diag(C): the tests assert min > 0, so that the oracle's clamp at 0 cannot hide a difference

The problems are those of tests/loo_oracle.py (its helpers are imported, not copied); the candidates are a
linspace(0, 23, n) product grid whose first three rows are replaced by training rows.  tests/test_ivr_host.py holds closed to
brute without a GPU; the GPU tests then trust closed where brute is too slow.
"""
import functools

import numpy as np
import torch

from oracle import gpim_oracle as O
from loo_oracle import JITTER, kp_from_u, pair, problem, scattered  # noqa: F401  (re-exported for the tests)


def grid(shape, X=None, hi=23.0):
    """(M, d) float64 tensor: the product grid of linspace(0, hi, n) per axis (row-major); with X its first three rows are
    replaced by the first three training rows (candidates that are already measured)"""
    axes = [np.linspace(0.0, hi, n) for n in shape]
    G = np.stack([g.reshape(-1) for g in np.meshgrid(*axes, indexing="ij")], axis=1)
    if X is not None:
        G[:3] = X[:3].numpy()
    return torch.from_numpy(np.ascontiguousarray(G))


def weights(M, seed):
    """random weights in [0, 2] with exact zeros at every fifth point"""
    w = np.random.default_rng(seed).uniform(0.0, 2.0, M)
    w[::5] = 0.0
    return w


def posterior_cov(kp, X, G, jitter=JITTER):
    """(C, noise): the latent posterior covariance of the rows G through a Cholesky factor of S in float64"""
    with torch.no_grad():
        K = kp.K(X).numpy().copy()
        Ks = kp.K(X, G).numpy()
        Kss = kp.K(G).numpy()
        noise = kp.noise.item()
    K[np.diag_indices(K.shape[0])] += jitter + noise
    W = np.linalg.solve(np.linalg.cholesky(K), Ks)
    C = Kss - W.T @ W
    return 0.5 * (C + C.T), noise


def latent_var(kp, X, G, jitter=JITTER):
    return np.diag(posterior_cov(kp, X, G, jitter)[0]).copy()


def closed(kp, X, G, w=None, jitter=JITTER):
    C, noise = posterior_cov(kp, X, G, jitter)
    w = np.ones(C.shape[0]) if w is None else np.asarray(w, dtype=np.float64)
    return (w[:, None] * C * C).sum(0) / (np.maximum(np.diag(C), 0.0) + noise + jitter)


def brute(kp, X, G, w=None, jitter=JITTER):
    M = G.shape[0]
    w = np.ones(M) if w is None else np.asarray(w, dtype=np.float64)
    y0 = torch.zeros(X.shape[0] + 1, dtype=torch.float64)
    before = O.ExactGP(X, y0[:-1], kp, jitter).predict(G)[1].numpy()
    a = np.empty(M)
    for j in range(M):
        after = O.ExactGP(torch.cat([X, G[j:j + 1]]), y0, kp, jitter).predict(G)[1].numpy()
        a[j] = np.sum(w * (before - after))
    return a


# (kind, N, grid shape): three kernels with less than one tile of candidates; two tiles, the second holding 2 columns;
# the same N in three dimensions
BRUTE_CASES = [("RBF", 40, (6, 5)), ("Matern52", 40, (6, 5)), ("RationalQuadratic", 40, (6, 5)), ("Matern52", 130, (13, 10)),
               ("Matern52", 130, (6, 5, 5))]


def case(kind, N, shape):
    """(kp, spec, u, X, y, G) of one case"""
    kp, spec, u, X, y = problem(kind, N, len(shape), False)
    return kp, spec, u, X, y, grid(shape, X)


@functools.lru_cache(maxsize=None)
def reference(kind, N, shape, how, wseed=None):
    """The reference of a case, computed once and shared: how = 'brute' or 'closed'; wseed: weights(M, wseed) or None"""
    kp, _, _, X, _, G = case(kind, N, shape)
    w = None if wseed is None else weights(G.shape[0], wseed)
    a = (brute if how == "brute" else closed)(kp, X, G, w)
    a.setflags(write=False)
    return a
