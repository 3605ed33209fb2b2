"""
Host oracle of the draws on a grid with missing points through the bordered reflection blocks (gpimhip_sample_border,
reconstructor.sample(method='border')), float64 numpy with every matrix explicit.

G: the completed grid (M points), o / m its observed / missing points, s = noise + jitter, 0 < d <= s,
A = K_GG + s I, V = A^-1 P_m, S = P_m^T V, E = A^-1 - V S^-1 V^T ( = (K_oo + s I)^-1 embedded in the grid).  Per draw:

    g    = U^T blockdiag(chol(K_b + d I)) z_p               the prior draw of pathwise_oracle
    r~   = 1_o (g + sqrt(s - d) z_e),  y~ = 1_o y
    beta = A^-1 [r~ | y~],  t = beta_m,  w = S^-1 t,  alpha~ = beta - V w      (alpha~ vanishes at the missing points)
    p    = (s - d) alpha~ - sqrt(s - d) z_e   at the observed points,   g + w   at the missing ones
    mean = y - s alpha~_y                     at the observed points,   - w_y   at the missing ones
    out  = mean + p  (+ sqrt(noise) z_n unless noiseless)

z = [z_p | z_e | z_n], each of width M and indexed by the grid point; the entries of z_e at missing points are ignored.
tests/test_border_sample_host.py holds this recipe to pathwise_oracle.draws with idx = the observed points.
"""
import numpy as np

import pathwise_oracle as PO


def observed(M, miss):
    obs = np.ones(M, dtype=bool)
    obs[np.asarray(miss, dtype=np.int64)] = False
    return obs


def pathwise_z(Z, M, miss):
    """The rows of Z in the layout of pathwise_oracle.draws with idx = the observed points: [z_p | z_e[idx] | z_n]."""
    idx = np.flatnonzero(observed(M, miss))
    Z = np.atleast_2d(Z)
    return np.concatenate([Z[:, :M], Z[:, M:2 * M][:, idx], Z[:, 2 * M:]], axis=1), idx


def pieces(P, blocks, miss):
    """A^-1, V, S and E as dense matrices."""
    M = blocks.M
    miss = np.asarray(miss, dtype=np.int64)
    A = PO.kmat(P, blocks.G, blocks.G) + P.s * np.eye(M)
    Ai = np.linalg.inv(A)
    Ai = 0.5 * (Ai + Ai.T)
    V = Ai[:, miss]
    S = V[miss, :]
    E = Ai - V @ np.linalg.solve(S, V.T)
    return {"A": A, "Ainv": Ai, "V": V, "S": S, "E": E}


def draws(P, blocks, miss, y, Z, noiseless, d=None):
    """The recipe for the rows Z (S, 2 M [+ M]) and the observations y (M, grid order; anything at the missing points).
    Returns dict: out (S, M), mean (M), p (S, M), g (S, M), alpha (S + 1, M) = alpha~ of the draws and of y, w (S + 1, m)."""
    d = P.jitter if d is None else float(d)
    s = P.s
    if not (0.0 < d <= s):
        raise ValueError("0 < d <= s")
    Z = np.atleast_2d(np.asarray(Z, dtype=np.float64))
    M, nS = blocks.M, Z.shape[0]
    assert Z.shape[1] == 2 * M + (0 if noiseless else M)
    miss = np.asarray(miss, dtype=np.int64)
    obs = observed(M, miss)
    Q = pieces(P, blocks, miss)
    sq = np.sqrt(s - d)
    g = blocks.prior_draw(P, d, Z[:, :M])
    ze = Z[:, M:2 * M]
    R = np.concatenate([np.where(obs[None, :], g + sq * ze, 0.0), np.where(obs, np.nan_to_num(y), 0.0)[None, :]])   # (S + 1, M)
    L = np.linalg.cholesky(Q["A"])
    beta = np.linalg.solve(L.T, np.linalg.solve(L, R.T)).T
    Ls = np.linalg.cholesky(Q["S"])
    w = np.linalg.solve(Ls.T, np.linalg.solve(Ls, beta[:, miss].T)).T          # (S + 1, m)
    alpha = beta - w @ Q["V"].T
    p = np.where(obs[None, :], (s - d) * alpha[:nS] - sq * ze, g)
    p[:, miss] += w[:nS]
    mean = np.where(obs, R[nS] - s * alpha[nS], 0.0)
    mean[miss] = -w[nS]
    out = mean[None, :] + p
    if not noiseless:
        out = out + np.sqrt(P.noise) * Z[:, 2 * M:]
    return {"out": out, "mean": mean, "p": p, "g": g, "alpha": alpha, "w": w}


def condition(P, blocks, d=None):
    """The condition number reported for a case: the largest among K_GG + s I on the completed grid (it bounds that of its
    principal submatrix K_oo + s I, and it is the matrix the explicit inverses go through) and the prior blocks K_b + d I."""
    d = P.jitter if d is None else float(d)
    return max(PO.cond_spd(PO.kmat(P, blocks.G, blocks.G) + P.s * np.eye(blocks.M)), blocks.condition(P, d))


def missing_sets(shape):
    """The missing sets of the host and GPU tests as {name: flat indices}: a single point off every mirror plane; a point on
    the mirror plane of an odd axis (grids that have one); a point together with its mirror image along the first reflected
    axis (the same representative q); about 10 % of the points at random."""
    shape = tuple(shape)
    M = int(np.prod(shape))
    flat = lambda ix: int(np.ravel_multi_index(tuple(ix), shape))
    one = [1] + [0] * (len(shape) - 1)
    sets = {"single": [flat(one)]}
    odd = [k for k, n in enumerate(shape) if n % 2 == 1]
    if odd:
        ix = list(one)
        ix[odd[0]] = shape[odd[0]] // 2
        sets["plane"] = [flat(ix)]
    mir = list(one)
    mir[0] = shape[0] - 1 - mir[0]
    sets["pair"] = sorted([flat(one), flat(mir)])
    sets["random"] = sorted(np.random.default_rng(M).choice(M, size=max(2, M // 10), replace=False).tolist())
    return {k: np.asarray(v, dtype=np.int64) for k, v in sets.items()}
