"""
Host oracles of the joint posterior draws of the multi-output GP (gpimhip_sample_vgp / gpimhip_sample_vgp_blocks,
vreconstructor.sample), float64.

* ``dense``: the posterior of the N T x N T model without any reduction -- mean and the full M T x M T covariance
      Sigma = B (x) K** + ((0 or S) + d S) (x) I - (B (x) K*^T) C^-1 (B (x) K*),      C = B (x) K + S (x) I
  from vgp_oracle.params_torch / kmat_torch (d: the draw jitter, relative to each task's noise).
* ``dense_blocks``: the same for the route through the reflection blocks of a fully observed grid, whose latent prior carries
  the jitter (tests/pathwise_oracle.py: Sigma_pw with idx = arange(M)):
      Kd = B (x) K + d S (x) I,      Sigma = Kd - Kd C^-1 Kd (+ S (x) I unless noiseless),      mean = mu + (B (x) K) C^-1 r
* ``Recipe``: what the engine computes -- B~ = S^-1/2 B S^-1/2 = Q diag(lambda) Q^T, T independent single-output draws of the
  latent blocks (variance lambda_t, noise 1, targets z_t = P^T (Y - mu)) mixed back, f_a = mu_a + s_a^1/2 sum_t Q_at h_t.
  ``eig='jacobi'`` restates the cyclic Jacobi iteration of csrc/vgp.hip (same pairs, same rotations), so that Q has the
  engine's column order and signs and a draw is the same function of z on both sides; ``eig='eigh'`` is numpy's.

Vectors over (point, task) are point-major with the task fastest, the layout of the engine's outputs.
"""
import numpy as np
import torch

import blocks_oracle as BO
import pathwise_oracle as PO
import vgp_oracle as VO

F64 = torch.float64


def params(u, T, n_ls, independent, bounds):
    mu, B, s, ls = VO.params_torch(torch.as_tensor(np.asarray(u, dtype=np.float64)), T, n_ls, independent, bounds)
    return mu.numpy().copy(), B.numpy().copy(), s.numpy().copy(), ls.numpy().copy()


def kmat(Xa, Xb, ls, kernel):
    return VO.kmat_torch(torch.as_tensor(np.asarray(Xa, dtype=np.float64)), torch.as_tensor(np.asarray(Xb, dtype=np.float64)),
                         torch.as_tensor(ls), kernel).numpy()


def _point_major(A, T, M):
    """(T M) task-major index -> (M T) point-major, on every axis of A."""
    perm = np.arange(T * M).reshape(T, M).T.reshape(-1)
    return A[perm] if A.ndim == 1 else A[np.ix_(perm, perm)]


def dense(u, X, Y, Xs, kernel, independent, bounds, noiseless, jitter, n_ls=None):
    """(mean (M, T), Sigma (M T, M T) point-major) of the joint route."""
    X, Y, Xs = (np.asarray(a, dtype=np.float64) for a in (X, Y, Xs))
    N, T = Y.shape
    M = Xs.shape[0]
    mu, B, s, ls = params(u, T, X.shape[1] if n_ls is None else n_ls, independent, bounds)
    K, Ks, Kss = kmat(X, X, ls, kernel), kmat(X, Xs, ls, kernel), kmat(Xs, Xs, ls, kernel)
    C = np.kron(B, K) + np.kron(np.diag(s), np.eye(N))
    L = np.linalg.cholesky(C)
    Cs = np.kron(B, Ks)                                            # (T N, T M)
    W = np.linalg.solve(L, Cs)
    r = (Y - mu[None, :]).T.reshape(-1)
    mean = mu[None, :] + (Cs.T @ np.linalg.solve(L.T, np.linalg.solve(L, r))).reshape(T, M).T
    diag = (0.0 if noiseless else s) + jitter * s
    Sig = np.kron(B, Kss) + np.kron(np.diag(diag * np.ones(T)), np.eye(M)) - W.T @ W
    return mean, _point_major(Sig, T, M)


def dense_blocks(u, G, Yg, kernel, independent, bounds, noiseless, jitter, n_ls=None):
    """(mean (M, T), Sigma (M T, M T) point-major) of the blocks route on the fully observed grid rows G (Yg in grid order)."""
    G, Yg = np.asarray(G, dtype=np.float64), np.asarray(Yg, dtype=np.float64)
    M, T = Yg.shape
    mu, B, s, ls = params(u, T, G.shape[1] if n_ls is None else n_ls, independent, bounds)
    K = kmat(G, G, ls, kernel)
    BK = np.kron(B, K)
    C = BK + np.kron(np.diag(s), np.eye(M))
    Kd = BK + jitter * np.kron(np.diag(s), np.eye(M))
    L = np.linalg.cholesky(C)
    W = np.linalg.solve(L, Kd)
    r = (Yg - mu[None, :]).T.reshape(-1)
    mean = mu[None, :] + (BK @ np.linalg.solve(L.T, np.linalg.solve(L, r))).reshape(T, M).T
    Sig = Kd - W.T @ W
    if not noiseless:
        Sig = Sig + np.kron(np.diag(s), np.eye(M))
    return mean, _point_major(Sig, T, M)


def strong_u(T, n_ls, independent, seed, identical=False):
    """A raw vector with a strong task covariance and little noise: eigenvalues of B~ of the order of 100."""
    o, _ = VO.layout(T, n_ls, independent)
    u = VO.random_u(T, n_ls, independent, seed)
    u[o["noise"]] = -2.5 + 0.3 * u[o["noise"]]
    u[o["global"]] = -2.5
    if independent:
        u[o["scale"]] = 2.0 + u[o["scale"]]
    else:
        u[o["F"]] = 3.0 * u[o["F"]] if T > 1 else 3.0
    if identical:               # the same row of F, diagonal and noise for every task: lambda has multiplicity T - 1
        for key in ("F", "rv", "noise", "mu"):
            u[o[key]] = u[o[key]][0]
    return u


def jacobi(A, sweeps=12):
    """Cyclic Jacobi as vgp_setup_kernel runs it: pairs (p, q) in row order, V from the identity; (diag, V)."""
    A = np.array(A, dtype=np.float64)
    T = A.shape[0]
    V = np.eye(T)
    for _ in range(sweeps):
        off = sum(A[p, q] ** 2 for p in range(T) for q in range(p + 1, T))
        if not off > 1e-40 * sum(A[p, p] ** 2 for p in range(T)):
            break
        for p in range(T - 1):
            for q in range(p + 1, T):
                apq = A[p, q]
                if apq == 0.0:
                    continue
                th = (A[q, q] - A[p, p]) / (2.0 * apq)
                t = 1.0 / (abs(th) + np.sqrt(th * th + 1.0))
                if th < 0.0:
                    t = -t
                c = 1.0 / np.sqrt(t * t + 1.0)
                sn = t * c
                if sn == 0.0:
                    continue
                tt = sn / c
                for k in range(T):
                    if k != p and k != q:
                        akp, akq = A[k, p], A[k, q]
                        A[k, p] = A[p, k] = c * akp - sn * akq
                        A[k, q] = A[q, k] = sn * akp + c * akq
                A[p, p], A[q, q] = A[p, p] - tt * apq, A[q, q] + tt * apq
                A[p, q] = A[q, p] = 0.0
                vp, vq = V[:, p].copy(), V[:, q].copy()
                V[:, p], V[:, q] = c * vp - sn * vq, sn * vp + c * vq
    return np.diag(A).copy(), V


class Recipe:
    """The block recipe at u: lam, Q, the projected targets Zt (N, T)."""

    def __init__(self, u, X, Y, kernel, independent, bounds, eig="jacobi", n_ls=None):
        self.X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
        self.N, self.T = Y.shape
        self.kernel = kernel
        self.mu, self.B, self.s, self.ls = params(u, self.T, self.X.shape[1] if n_ls is None else n_ls, independent, bounds)
        Bt = self.B / np.sqrt(np.outer(self.s, self.s))
        if eig == "jacobi":
            self.lam, self.Q = jacobi(Bt)
        else:
            self.lam, self.Q = np.linalg.eigh(Bt)
        self.Zt = (Y - self.mu[None, :]) @ (self.Q / np.sqrt(self.s)[:, None])

    def mix(self, H):
        """H (T, ..., M) of the latent blocks -> (..., M, T): mu_a + s_a^1/2 sum_t Q_at H[t]."""
        return self.mu + np.sqrt(self.s) * np.einsum("at,t...->...a", self.Q, H)

    # ---- the joint route: per block the factor of the joint covariance of [X; Xs]
    def joint(self, Xs, noiseless, jitter):
        """dict: mean (M, T), var (M, T) (noise included, jitter excluded), bmean (T, M), D (T, M, M) lower factors."""
        Xs = np.asarray(Xs, dtype=np.float64)
        N, M, T = self.N, Xs.shape[0], self.T
        XX = np.concatenate([self.X, Xs])
        K = kmat(XX, XX, self.ls, self.kernel)
        add = np.concatenate([np.ones(N), np.full(M, (0.0 if noiseless else 1.0) + jitter)])
        bmean, bvar, D = np.empty((T, M)), np.empty((T, M)), np.empty((T, M, M))
        for t in range(T):
            L = np.linalg.cholesky(self.lam[t] * K + np.diag(add))
            zf = np.linalg.solve(L[:N, :N], self.Zt[:, t])
            bmean[t] = L[N:, :N] @ zf
            D[t] = L[N:, N:]
            bvar[t] = (D[t] ** 2).sum(1) - add[N:] + 1.0
        mean = self.mix(bmean)
        var = self.s * np.einsum("at,tm->ma", self.Q ** 2, bvar)
        return {"mean": mean, "var": var, "bmean": bmean, "D": D}

    def joint_draws(self, J, Z):
        """Z (T, S, M) -> (S, M, T)"""
        H = J["bmean"][:, None, :] + np.einsum("tij,tsj->tsi", J["D"], np.asarray(Z, dtype=np.float64))
        return self.mix(H)

    def joint_factor(self, J):
        """A (M T, T M): draws - mean = A z, rows point-major (task fastest), columns block-major (z of block t, point j)."""
        T, M = self.T, J["D"].shape[1]
        A = np.einsum("a,at,tij->iatj", np.sqrt(self.s), self.Q, J["D"])
        return A.reshape(M * T, T * M)

    # ---- the blocks route: blocks_oracle.draws per latent block (variance lambda_t, s = 1), mixed
    def blocks_draws(self, blocks, Z, noiseless, jitter):
        """The observed rows must be blocks.G in grid order.  Z (T, S, 2 M [+ M]) -> dict: out (S, M, T), mean (M, T)."""
        Z = np.asarray(Z, dtype=np.float64)
        T, S, M = self.T, Z.shape[1], blocks.M
        H, bmean = np.empty((T, S, M)), np.empty((T, M))
        d = len(self.ls) if len(self.ls) > 1 else blocks.d
        for t in range(T):
            P = PO.Params(self.kernel, self.lam[t], np.broadcast_to(self.ls, (d,)).copy(), 1.0, 1.0, 0.0)
            R = BO.draws(P, blocks, self.Zt[:, t], Z[t], noiseless, d=jitter)
            H[t], bmean[t] = R["out"], R["mean"]
        return {"out": self.mix(H), "mean": self.mix(bmean)}
