"""
Host oracle of the posterior draws of the spectral-mixture GP (gpimhip_sample_sm / _pathwise / _blocks,
skreconstructor(kernel='Spectral').sample), float64 numpy with np.linalg.cholesky for every factor.
The covariance is sm_oracle.kmat; the grid structure (U, zsrc, wts, present) is pathwise_oracle.Blocks with the covariance of
the blocks overridden.  The model has a constant mean c and no jitter of its own: s = noise, right-hand sides are y - c, and c
is added to the mean and to every draw.

    joint      chol of the joint covariance of [X; Xs] with noise on the N training rows and (noiseless ? 0 : noise) + d on
               the M test rows; out = mean + L22 z
    pathwise   g = U^T blockdiag_b(chol(K_b + d I)) z_p;  r = g[idx] + sqrt(s - d) z_e;  a = (K + s I)^-1 r
               out = c + mean0 + g - (K_GX a + d scatter(idx, a))  (+ sqrt(noise) z_n),  mean0 = K_GX (K + s I)^-1 (y - c)
    blocks     per block: c_b = chol(K_b + d I) z_b, [alpha_b | alpha_y,b] = (K_b + s I)^-1 [c_b + sqrt(s - d) e_b | ys_b],
               out = c + U^T [ys_b - s alpha_y,b + (s - d) alpha_b - sqrt(s - d) e_b]  (+ sqrt(noise) z_n)
               with e_b = (U z_e)_b, ys_b = (U (y - c))_b

Shared by tests/test_sm_sample_host.py and tests/test_gpu_spectral_sample.py, which also take the two measured host figures
below from here.
"""
import numpy as np
import torch

import pathwise_oracle as PO
import sm_oracle as SO

# Measured by tests/test_sm_sample_host.py over its cases (6x5 with N = 7 and 30, 13x10 with N = 40 and Q = 16 isotropic,
# 4x3x4 with N = 9 isotropic; random_u and narrow_u), printed there with -s:
#   HOST_DISCREPANCY_OVER_SW  max |A A^T - Sigma_pw| / sum w between the recipe applied to the identity and the explicit
#                             formula (measured 4.7e-16 ... 7.1e-15)
#   COV_SHIFT_OVER_D          max |Sigma_pw - Sigma| / d, Sigma the covariance of the joint route
#                             (measured 1.588 ... 1.991)
# The GPU tests scale the first; the host test asserts that they still describe what it measures.
HOST_DISCREPANCY_OVER_SW = 7.2e-15
COV_SHIFT_OVER_D = 2.0
JITTER = 1e-5


def narrow_u(Q, D, seed):
    """A raw vector with trained-like narrow spectral peaks (sm_oracle.random_u gives nearly white kernels whose condition
    numbers stay below 5): means 0.05 .. 0.3 and scales 0.02 .. 0.06 per unit of x, noise 1e-4 + softplus(-4) = 0.018."""
    rng = np.random.default_rng(seed)
    u = np.zeros(2 + Q * (2 * D + 1))
    u[0] = 0.3 * rng.normal()
    u[1:1 + Q] = 0.5 * rng.normal(size=Q) - 1.0
    u[1 + Q:1 + Q + Q * D] = np.log(np.expm1(rng.uniform(0.05, 0.3, Q * D)))
    u[1 + Q + Q * D:1 + Q + 2 * Q * D] = np.log(np.expm1(rng.uniform(0.02, 0.06, Q * D)))
    u[-1] = -4.0
    return u


GENERATORS = {"random_u": SO.random_u, "narrow_u": narrow_u}


class Params:
    """The model at the raw vector u: c, sum w, noise, the draw's jitter d, and the covariance."""

    def __init__(self, u, Q, D, jitter=JITTER):
        self.u, self.Q, self.D = np.asarray(u, dtype=np.float64), int(Q), int(D)
        c, w, _, _, noise = SO.split(torch.as_tensor(self.u), self.Q, self.D)
        self.c, self.var, self.noise, self.jitter = float(c), float(w.sum()), float(noise), float(jitter)
        self.s = self.noise                                     # (the model has no jitter of its own)

    def kmat(self, A, B):
        return SO.kmat(np.ascontiguousarray(A, dtype=np.float64), np.ascontiguousarray(B, dtype=np.float64), self.u, self.Q,
                       self.D).numpy()


class Blocks(PO.Blocks):
    """pathwise_oracle.Blocks with the blocks of the spectral-mixture covariance: prior_draw and condition are inherited."""

    def prior_blocks(self, P, d):
        out = []
        for b in range(self.B):
            acc = np.zeros((self.Nq, self.Nq))
            for g in range(self.B):
                Xm = self.Xq.copy()
                for j, k in enumerate(self.dims):
                    if (g >> j) & 1:
                        Xm[:, k] = self.twoc[k] - Xm[:, k]
                chi = -1.0 if bin(g & b).count("1") & 1 else 1.0
                acc += chi * P.kmat(self.Xq, Xm)
            w = self.wts[b]
            Kb = acc * w[:, None] * w[None, :]
            pr = self.present[b]
            Kb[~pr, :] = 0.0
            Kb[:, ~pr] = 0.0
            Kb[np.arange(self.Nq), np.arange(self.Nq)] += np.where(pr, d, 1.0)
            out.append(Kb)
        return out


def _check_d(P, d, positive=True):
    """The draw's jitter under the rule of the method: 0 < d <= noise, or d >= 0 for the joint route."""
    d = P.jitter if d is None else float(d)
    if positive and not (0.0 < d <= P.s):
        raise ValueError("0 < d <= noise")
    if not positive and not (0.0 <= d < np.inf):
        raise ValueError("d >= 0")
    return d


def _solver(K):
    L = np.linalg.cholesky(K)
    return lambda R: np.linalg.solve(L.T, np.linalg.solve(L, R))


# ---------------------------------------------------------------------------------------------- joint
def joint_matrix(P, X, Xs, noiseless, d):
    N, M = len(X), len(Xs)
    XX = np.concatenate([X, Xs])
    J = P.kmat(XX, XX)
    J = 0.5 * (J + J.T)
    J[np.arange(N + M), np.arange(N + M)] += np.concatenate([np.full(N, P.s), np.full(M, (0.0 if noiseless else P.noise) + d)])
    return J


def joint_factor(P, X, Xs, noiseless, d=None):
    """chol of the joint covariance of [X; Xs] with the two diagonal terms on their segments (as sample_oracle.joint_factor)."""
    return np.linalg.cholesky(joint_matrix(P, X, Xs, noiseless, _check_d(P, d, positive=False)))


def joint_draws(P, X, y, Xs, Z, noiseless, d=None):
    """out (S, M) = mean + L22 z for the rows Z (S, M); also mean (M), var (M: noise included, jitter excluded), cond."""
    d = _check_d(P, d, positive=False)
    N = len(X)
    J = joint_matrix(P, X, Xs, noiseless, d)
    L = np.linalg.cholesky(J)
    z = np.linalg.solve(L[:N, :N], np.asarray(y, dtype=np.float64) - P.c)
    mean = P.c + L[N:, :N] @ z
    L22 = L[N:, N:]
    var = (L22 ** 2).sum(1) - ((0.0 if noiseless else P.noise) + d) + P.noise
    out = mean[None, :] + np.atleast_2d(Z) @ L22.T
    return {"out": out, "mean": mean, "var": var, "cond": PO.cond_spd(J)}


# ---------------------------------------------------------------------------------------------- pathwise
def draws(P, blocks, idx, y, Z, noiseless, d=None, scatter=True):
    """The pathwise recipe for the rows Z (S, M + N [+ M]) = [z_p | z_e | z_n].  Returns dict: out (S, M), mean (M, c
    included), p (S, M) = out without mean and grid noise, g (S, M), alpha (S, N)."""
    d = _check_d(P, d)
    Z = np.atleast_2d(np.asarray(Z, dtype=np.float64))
    M, N = blocks.M, len(idx)
    assert Z.shape[1] == M + N + (0 if noiseless else M)
    X = blocks.G[idx]
    g = blocks.prior_draw(P, d, Z[:, :M])
    r = g[:, idx] + np.sqrt(P.s - d) * Z[:, M:M + N]
    solve = _solver(P.kmat(X, X) + P.s * np.eye(N))
    alpha = solve(r.T).T
    Kgx = P.kmat(blocks.G, X)
    upd = alpha @ Kgx.T
    if scatter:
        upd[:, idx] += d * alpha
    p = g - upd
    mean = P.c + Kgx @ solve(np.asarray(y, dtype=np.float64) - P.c)
    out = mean[None, :] + p
    if not noiseless:
        out = out + np.sqrt(P.noise) * Z[:, M + N:]
    return {"out": out, "mean": mean, "p": p, "g": g, "alpha": alpha}


def probe_matrix(P, blocks, idx, d=None, scatter=True):
    """A (M, M + N) with p = A z: the recipe applied to the columns of the identity."""
    M, N = blocks.M, len(idx)
    return draws(P, blocks, idx, np.full(N, P.c), np.eye(M + N), True, d, scatter)["p"].T.copy()


def _sigma(P, blocks, idx, d, scatter):
    d = _check_d(P, d)
    M, N = blocks.M, len(idx)
    X = blocks.G[idx]
    C = P.kmat(blocks.G, X)
    if scatter:
        C[idx, np.arange(N)] += d
    A = np.linalg.inv(P.kmat(X, X) + P.s * np.eye(N))
    A = 0.5 * (A + A.T)
    return P.kmat(blocks.G, blocks.G) + d * np.eye(M) - C @ A @ C.T


def sigma_pathwise(P, blocks, idx, d=None):
    """Sigma_pw = K_GG + d I - (K_GX + d P)(K + s I)^-1 (K_GX + d P)^T, the covariance of p."""
    return _sigma(P, blocks, idx, d, True)


def sigma_joint(P, blocks, idx, d=None):
    """Sigma of the joint route, noiseless: K_GG - K_GX (K + s I)^-1 K_XG + d I."""
    return _sigma(P, blocks, idx, d, False)


def condition(P, blocks, idx, d=None):
    """The condition number reported for a pathwise case: the largest among K + s I and the prior blocks K_b + d I."""
    d = _check_d(P, d)
    X = blocks.G[idx]
    return max(PO.cond_spd(P.kmat(X, X) + P.s * np.eye(len(idx))), blocks.condition(P, d))


# ---------------------------------------------------------------------------------------------- blocks
def blocks_draws(P, blocks, y, Z, noiseless, d=None):
    """The block recipe for the rows Z (S, 2 M [+ M]) = [z_p | z_e | z_n] and the observations y (M, grid order).  Returns
    dict: out (S, M), mean (M, c included), cond (the largest among the blocks K_b + d I and K_b + s I)."""
    d = _check_d(P, d)
    s = P.s
    Z = np.atleast_2d(np.asarray(Z, dtype=np.float64))
    M, S = blocks.M, Z.shape[0]
    assert Z.shape[1] == 2 * M + (0 if noiseless else M)
    U2 = blocks.U2()
    fwd = lambda v: (np.asarray(v, dtype=np.float64) @ U2.T).reshape(np.shape(v)[:-1] + (blocks.B, blocks.Nq))
    E, ys = fwd(Z[:, M:2 * M]), fwd(np.asarray(y, dtype=np.float64) - P.c)
    sq = np.sqrt(s - d)
    p, mean, cond = np.zeros((S, M)), np.zeros(M), 0.0
    for b, Cb in enumerate(blocks.prior_blocks(P, d)):
        pr = blocks.present[b]
        zb = np.where(pr[None, :], Z[:, blocks.zsrc[b]], 0.0)
        c = zb @ np.linalg.cholesky(Cb).T
        Tb = Cb + np.diag(np.where(pr, s - d, 0.0))
        solve = _solver(Tb)
        al = solve((c + sq * E[:, b]).T).T
        ay = solve(ys[b])
        p += ((s - d) * al - sq * E[:, b]) @ blocks.U[b]
        mean += (ys[b] - s * ay) @ blocks.U[b]
        cond = max(cond, PO.cond_spd(Cb[np.ix_(pr, pr)]), PO.cond_spd(Tb[np.ix_(pr, pr)]))
    mean = mean + P.c
    out = mean[None, :] + p
    if not noiseless:
        out = out + np.sqrt(P.noise) * Z[:, 2 * M:]
    return {"out": out, "mean": mean, "cond": cond}
