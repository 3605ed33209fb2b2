"""
Host oracle of the pathwise posterior draws (gpimhip_sample_pathwise, reconstructor.sample(method='pathwise'); DESIGN.md
section 16), float64 numpy:

    g   = U^T blockdiag_b(chol(K_b + d I)) z_p          a prior draw on the complete grid G,  g ~ N(0, K_GG + d I)
    r   = g[idx] + sqrt(s - d) z_e                       r ~ N(0, K + s I),  s = noise + jitter
    a   = (K + s I)^-1 r
    p   = g - (K_GX a + d scatter(idx, a))
    out = mean + p  (+ sqrt(noise) z_n unless noiseless),   mean = K_GX (K + s I)^-1 y

with np.linalg.cholesky for every factor.  U is the basis change of gprutils.reflection_blocks, built here entry by entry
(tests/test_pathwise_host.py holds it to reflection_blocks); K_b are the reflection blocks by their defining sum over the
mirror images.  z_p is indexed by the grid point: row p of block b takes z_p[flat(gamma_b p)], gamma_b the reflection of the
axes whose sign is -1 in b -- a bijection of the rows that exist onto G.  Shared by tests/test_pathwise_host.py and
tests/test_gpu_pathwise.py, which also take the two measured host figures below from here.
"""
import numpy as np

from gpim_amd import gprutils

# Measured by tests/test_pathwise_host.py over its cases (6x5, 5x5, 8x8, 4x3x4; three kernels), printed there with -s:
#   HOST_DISCREPANCY  max |A A^T - Sigma_pw| between the recipe applied to the identity and the explicit formula
#                     (measured 1.04e-15 ... 1.86e-15)
#   COV_SHIFT_OVER_D  max |Sigma_pw - Sigma| / d, Sigma the covariance of the joint route
#                     (measured 1.777 ... 1.916)
# The GPU tests scale them; the host test asserts that they still describe what it measures.
HOST_DISCREPANCY = 1.9e-15
COV_SHIFT_OVER_D = 1.92


class Params:
    """Constrained hyper-parameters of one model: kind, variance, lengthscale per dimension, noise, alpha (RQ), jitter."""

    def __init__(self, kind, var, ls, noise, alpha=1.0, jitter=1e-5):
        self.kind, self.var, self.ls = kind, float(var), np.asarray(ls, dtype=np.float64).reshape(-1)
        self.noise, self.alpha, self.jitter = float(noise), float(alpha), float(jitter)

    @property
    def s(self):
        return self.noise + self.jitter

    @classmethod
    def from_oracle(cls, kp, d, jitter):
        """From an oracle.gpim_oracle.KernelParams (the GPU tests hold the same values in a KernelSpec / u pair)."""
        ls = np.broadcast_to(kp.lengthscale.detach().numpy().reshape(-1), (d,)).copy()
        alpha = float(kp.scale_mixture.detach()) if kp.kind == "RationalQuadratic" else 1.0
        return cls(kp.kind, float(kp.variance.detach()), ls, float(kp.noise.detach()), alpha, jitter)


def kmat(P, A, B):
    """k(A, B) with the algebraic forms of csrc/kfun.hpp; the squared distance from the coordinate differences."""
    a, b = np.asarray(A, dtype=np.float64) / P.ls, np.asarray(B, dtype=np.float64) / P.ls
    r2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    if P.kind == "RBF":
        return P.var * np.exp(-0.5 * r2)
    if P.kind == "Matern52":
        s5r = np.sqrt(5.0) * np.sqrt(r2 + 1e-12)
        return P.var * (1.0 + s5r + (5.0 / 3.0) * r2) * np.exp(-s5r)
    if P.kind == "RationalQuadratic":
        return P.var * (1.0 + (0.5 / P.alpha) * r2) ** (-P.alpha)
    raise KeyError(P.kind)


def cond_spd(K):
    """The 2-norm condition number of a symmetric positive definite matrix: the ratio of its extreme eigenvalues."""
    w = np.linalg.eigvalsh(K)
    return float(w[-1] / w[0])


def full_grid(shape):
    """(Xgrid (d, *shape), rows (M, d)) of the index grid, what utils.get_full_grid returns for an array of that shape."""
    Xg = np.array(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"))
    return Xg, Xg.reshape(len(shape), -1).T.copy()


class Blocks:
    """The reflection structure of a complete grid: everything below is a function of the grid alone."""

    def __init__(self, Xgrid):
        Xgrid = np.asarray(Xgrid, dtype=np.float64)
        self.d, self.shape = Xgrid.shape[0], tuple(Xgrid.shape[1:])
        self.G = Xgrid.reshape(self.d, -1).T.copy()
        self.M = self.G.shape[0]
        axes, _ = gprutils.grid_axes(Xgrid)
        S = gprutils.reflection_blocks(Xgrid, np.zeros(self.shape), axes)
        self.S, self.dims, self.B, self.Xq = S, S["dims"], S["B"], S["Xq"]
        self.twoc = np.asarray(S["twoc"][:self.d], dtype=np.float64)
        self.Nq = self.Xq.shape[0]
        self.wts = S["wts"] if S["wts"] is not None else np.ones((self.B, self.Nq))
        self.present = self.wts > 0
        fshape = tuple((n + 1) // 2 if k in self.dims else n for k, n in enumerate(self.shape))
        fidx = np.indices(fshape).reshape(self.d, -1)                         # multi-index of every domain point
        # zsrc[b, p]: flat grid index of gamma_b p
        self.zsrc = np.zeros((self.B, self.Nq), dtype=np.int64)
        for b in range(self.B):
            ix = fidx.copy()
            for j, k in enumerate(self.dims):
                if (b >> j) & 1:
                    ix[k] = self.shape[k] - 1 - ix[k]
            self.zsrc[b] = np.ravel_multi_index(tuple(ix), self.shape)
        # U[b, p, i]: the coefficient of e_i in basis vector (b, p): chi_b(gamma_i) sqrt(|Stab_p|) / sqrt(B) at i = gamma_i p
        full = np.indices(self.shape).reshape(self.d, -1)
        gam = np.zeros(self.M, dtype=np.int64)
        for j, k in enumerate(self.dims):
            gam |= (full[k] > (self.shape[k] - 1) // 2).astype(np.int64) << j
        rep = S["rep"]
        stab = 1.0 / self.wts[0] ** 2                          # |Stab_p| (every point exists in block 0)
        self.U = np.zeros((self.B, self.Nq, self.M))
        for b in range(self.B):
            chi = np.ones(self.M)
            for j in range(len(self.dims)):
                if (b >> j) & 1:
                    chi = np.where((gam >> j) & 1, -chi, chi)
            ok = self.present[b, rep]
            ii = np.flatnonzero(ok)
            self.U[b, rep[ii], ii] = chi[ii] * np.sqrt(stab[rep[ii]]) / np.sqrt(self.B)

    def U2(self):
        """U as a (B Nq, M) matrix, the rows of points that do not exist in their block are zero."""
        return self.U.reshape(self.B * self.Nq, self.M)

    def prior_blocks(self, P, d):
        """K_b + d I per block: K_b[p, q] = w_p w_q sum_g chi_b(g) k(p, g q); rows of absent points are identity rows."""
        out = []
        for b in range(self.B):
            acc = np.zeros((self.Nq, self.Nq))
            for g in range(self.B):
                Xm = self.Xq.copy()
                for j, k in enumerate(self.dims):
                    if (g >> j) & 1:
                        Xm[:, k] = self.twoc[k] - Xm[:, k]
                chi = -1.0 if bin(g & b).count("1") & 1 else 1.0
                acc += chi * kmat(P, self.Xq, Xm)
            w = self.wts[b]
            Kb = acc * w[:, None] * w[None, :]
            pr = self.present[b]
            Kb[~pr, :] = 0.0
            Kb[:, ~pr] = 0.0
            Kb[np.arange(self.Nq), np.arange(self.Nq)] += np.where(pr, d, 1.0)
            out.append(Kb)
        return out

    def prior_draw(self, P, d, Zp):
        """g (S, M) = U^T blockdiag(chol(K_b + d I)) z for the rows Zp (S, M) of standard normals."""
        Zp = np.atleast_2d(Zp)
        g = np.zeros((Zp.shape[0], self.M))
        for b, Kb in enumerate(self.prior_blocks(P, d)):
            L = np.linalg.cholesky(Kb)
            zb = np.where(self.present[b][None, :], Zp[:, self.zsrc[b]], 0.0)       # (S, Nq)
            g += (zb @ L.T) @ self.U[b]
        return g

    def condition(self, P, d):
        """The largest 2-norm condition number among the prior blocks K_b + d I (rows of absent points left out)."""
        return max(cond_spd(Kb[np.ix_(self.present[b], self.present[b])]) for b, Kb in enumerate(self.prior_blocks(P, d)))


def draws(P, blocks, idx, y, Z, noiseless, d=None, scatter=True):
    """The recipe for the rows Z (S, M + N [+ M]) = [z_p | z_e | z_n].  Returns dict: out (S, M), mean (M), p (S, M) = out
    without mean and grid noise, g (S, M), alpha (S, N).  scatter=False leaves the d scatter(idx, alpha) term out."""
    d = P.jitter if d is None else float(d)
    if not (0.0 < d <= P.s):
        raise ValueError("0 < d <= s")
    Z = np.atleast_2d(np.asarray(Z, dtype=np.float64))
    M, N = blocks.M, len(idx)
    assert Z.shape[1] == M + N + (0 if noiseless else M)
    X = blocks.G[idx]
    g = blocks.prior_draw(P, d, Z[:, :M])
    r = g[:, idx] + np.sqrt(P.s - d) * Z[:, M:M + N]
    Kt = kmat(P, X, X) + P.s * np.eye(N)
    L = np.linalg.cholesky(Kt)
    solve = lambda R: np.linalg.solve(L.T, np.linalg.solve(L, R))
    alpha = solve(r.T).T                                       # (S, N)
    Kgx = kmat(P, blocks.G, X)
    upd = alpha @ Kgx.T
    if scatter:
        upd[:, idx] += d * alpha
    p = g - upd
    mean = Kgx @ solve(np.asarray(y, dtype=np.float64))
    out = mean[None, :] + p
    if not noiseless:
        out = out + np.sqrt(P.noise) * Z[:, M + N:]
    return {"out": out, "mean": mean, "p": p, "g": g, "alpha": alpha}


def probe_matrix(P, blocks, idx, d=None, scatter=True):
    """A (M, M + N) with p = A z: the recipe applied to the columns of the identity."""
    M, N = blocks.M, len(idx)
    R = draws(P, blocks, idx, np.zeros(N), np.eye(M + N), True, d, scatter)
    return R["p"].T.copy()


def sigma_pathwise(P, blocks, idx, d=None):
    """Sigma_pw = K_GG + d I - (K_GX + d P)(K + s I)^-1 (K_GX + d P)^T, the covariance of p."""
    d = P.jitter if d is None else float(d)
    M, N = blocks.M, len(idx)
    X = blocks.G[idx]
    C = kmat(P, blocks.G, X)
    C[idx, np.arange(N)] += d
    A = np.linalg.inv(kmat(P, X, X) + P.s * np.eye(N))
    A = 0.5 * (A + A.T)
    return kmat(P, blocks.G, blocks.G) + d * np.eye(M) - C @ A @ C.T


def sigma_joint(P, blocks, idx, d=None):
    """Sigma of the joint route, noiseless: K_GG - K_GX (K + s I)^-1 K_XG + d I."""
    d = P.jitter if d is None else float(d)
    X = blocks.G[idx]
    C = kmat(P, blocks.G, X)
    A = np.linalg.inv(kmat(P, X, X) + P.s * np.eye(len(idx)))
    A = 0.5 * (A + A.T)
    return kmat(P, blocks.G, blocks.G) + d * np.eye(blocks.M) - C @ A @ C.T


def condition(P, blocks, idx, d=None):
    """The condition number reported for a case: the largest among K + s I and the prior blocks K_b + d I."""
    d = P.jitter if d is None else float(d)
    X = blocks.G[idx]
    return max(cond_spd(kmat(P, X, X) + P.s * np.eye(len(idx))), blocks.condition(P, d))
