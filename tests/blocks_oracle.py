"""
Host oracle of the draws on a fully observed grid (gpimhip_sample_blocks, reconstructor.sample(method='blocks'); DESIGN.md
section 17), float64 numpy.  With an observation on every grid point the recipe of tests/pathwise_oracle.py is block diagonal
in the grid's reflection basis U; per block b, s = noise + jitter and 0 < d <= s:

    c_b = chol(K_b + d I) z_b                          z_b = z_p[zsrc[b]]            (the prior draw, as pathwise_oracle)
    r_b = c_b + sqrt(s - d) e_b                        e_b = (U z_e)_b,  ys_b = (U y)_b
    [alpha_b | alpha_y,b] = (K_b + s I)^-1 [r_b | ys_b]
    p_b    = (s - d) alpha_b - sqrt(s - d) e_b         ( = c_b - (K_b + d I) alpha_b )
    mean_b = ys_b - s alpha_y,b                        ( = K_b alpha_y,b )
    out    = U^T [mean_b + p_b]  (+ sqrt(noise) z_n unless noiseless)

Rows of points that do not exist in a block are identity rows with zero right-hand sides.  U, zsrc and the blocks K_b come from
pathwise_oracle.Blocks; tests/test_blocks_host.py holds this recipe to pathwise_oracle.draws(..., idx=arange(M)).
"""
import numpy as np


def forward(blocks, v):
    """(U v) as (B, Nq) for one vector, (S, B, Nq) for rows of vectors; zero where the point is absent from the block."""
    v = np.asarray(v, dtype=np.float64)
    return (v @ blocks.U2().T).reshape(v.shape[:-1] + (blocks.B, blocks.Nq))


def draws(P, blocks, y, Z, noiseless, d=None):
    """The recipe for the rows Z (S, 2 M [+ M]) = [z_p | z_e | z_n] and the observations y (M, grid order).
    Returns dict: out (S, M), mean (M), p (S, M) = out without mean and grid noise."""
    d = P.jitter if d is None else float(d)
    s = P.s
    if not (0.0 < d <= s):
        raise ValueError("0 < d <= s")
    Z = np.atleast_2d(np.asarray(Z, dtype=np.float64))
    M, S = blocks.M, Z.shape[0]
    assert Z.shape[1] == 2 * M + (0 if noiseless else M)
    E, ys = forward(blocks, Z[:, M:2 * M]), forward(blocks, y)
    sq = np.sqrt(s - d)
    p, mean = np.zeros((S, M)), np.zeros(M)
    for b, Cb in enumerate(blocks.prior_blocks(P, d)):
        pr = blocks.present[b]
        zb = np.where(pr[None, :], Z[:, blocks.zsrc[b]], 0.0)                 # (S, Nq)
        c = zb @ np.linalg.cholesky(Cb).T
        Tb = Cb + np.diag(np.where(pr, s - d, 0.0))
        L = np.linalg.cholesky(Tb)
        solve = lambda R: np.linalg.solve(L.T, np.linalg.solve(L, R))
        al = solve((c + sq * E[:, b]).T).T
        ay = solve(ys[b])
        p += ((s - d) * al - sq * E[:, b]) @ blocks.U[b]
        mean += (ys[b] - s * ay) @ blocks.U[b]
    out = mean[None, :] + p
    if not noiseless:
        out = out + np.sqrt(P.noise) * Z[:, 2 * M:]
    return {"out": out, "mean": mean, "p": p}
