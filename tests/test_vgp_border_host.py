"""CPU checks of the multi-output GP's border solver (vreconstructor on incomplete grids): the loss,
gradient, predictive mean and variance restated from gprutils.border_blocks_multi -- per task the 2^r reflection blocks
lambda_t K_b + I of the completed grid, corrected by the border S_t = (A_t^-1)_mm of the M missing points -- against the
dense restatement of tests/vgp_oracle.py (autograd) on the observed rows."""
import math

import numpy as np
import pytest

import vgp_oracle as V
import test_vgp_refl_host as R
from gpim_amd import gprutils


def masked(grid, T, frac, seed, data_seed):
    """A grid of test_vgp_refl_host with max(1, frac n) pixels removed: (X, Y, Xn, Yn, obs)."""
    X, Y, _ = R.grid_data(grid, T, seed=data_seed)
    d = X.shape[0]
    n = Y[..., 0].size
    miss = np.random.default_rng(seed).choice(n, max(1, int(round(frac * n))), replace=False)
    Yn = Y.copy().reshape(-1, T)
    Yn[miss] = np.nan
    Xn = X.copy().reshape(d, -1)
    Xn[:, miss] = np.nan
    obs = np.ones(n, dtype=bool)
    obs[miss] = False
    return X, Y, Xn.reshape(X.shape), Yn.reshape(Y.shape), obs


def _task_border(S, blocks, P, mu, lam, t):
    """Task t: the blocks' inverses, alpha, z, Cholesky factors, and the border's L_S, v, Y_b."""
    B, q_, coef = S["B"], S["q"], S["coef"]
    Minv, alpha, Zs, Ls = [], [], [], []
    for b, (K, dK, w) in enumerate(blocks):
        present = w != 0
        z = P[:, t] @ (S["ys"][:, b] - mu[:, None] * S["ones"][b][None, :])
        z[~present] = 0.0
        A = lam[t] * K + np.eye(K.shape[0])
        A[~present, :] = 0.0
        A[:, ~present] = 0.0
        A[~present, ~present] = 1.0
        Mi = np.linalg.inv(A)
        Minv.append(Mi)
        alpha.append(Mi @ z)
        Zs.append(z)
        Ls.append(np.linalg.cholesky(A))
    St = sum(np.outer(coef[b], coef[b]) * Minv[b][np.ix_(q_, q_)] for b in range(B))
    LS = np.linalg.cholesky(St)
    v = np.linalg.solve(LS, sum(coef[b] * alpha[b][q_] for b in range(B)))
    Yb = [np.linalg.solve(LS, (Minv[b][:, q_] * coef[b][None, :]).T).T for b in range(B)]
    return Minv, alpha, Zs, Ls, LS, v, Yb


def border_loss_grad(S, u, T, kernel, independent, bounds, isotropic):
    """section 12's loss and gradient from the corrected beta and the corrected inverses."""
    d = S["Xq"].shape[1]
    n_ls = 1 if isotropic else d
    o, P_len = V.layout(T, n_ls, independent)
    (mu, Bm, s, l, ls, lam, Q, P), blocks = R.refl_model(S, u, T, kernel, independent, bounds, isotropic)
    B, N = S["B"], S["n_obs"]
    lg = qd = 0.0
    trMK, trM = np.zeros(T), np.zeros(T)
    gl = np.zeros(n_ls)
    H, G, sig = np.zeros((T, T)), np.zeros((T, T)), np.zeros(T)
    betas = np.zeros((T, B, S["Xq"].shape[0]))
    for t in range(T):
        Minv, alpha, Zs, Ls, LS, v, Yb = _task_border(S, blocks, P, mu, lam, t)
        lg += sum(np.log(np.diag(L)).sum() for L in Ls) + np.log(np.diag(LS)).sum()
        for b, (K, dK, w) in enumerate(blocks):
            present = w != 0
            beta = alpha[b] - Yb[b] @ v
            M = Minv[b] - Yb[b] @ Yb[b].T
            betas[t, b] = beta
            qd += Zs[b] @ beta
            trMK[t] += (M * K).sum()
            trM[t] += np.trace(M[np.ix_(present, present)])
            for k in range(n_ls):
                gl[k] += 0.5 * lam[t] * ((M * dK[k]).sum() - beta @ dK[k] @ beta)
    for b, (K, dK, w) in enumerate(blocks):
        bb = betas[:, b]
        H += bb @ bb.T
        G += bb @ K @ bb.T
        sig += bb @ S["ones"][b]
    gB = 0.5 * (P @ np.diag(trMK) @ P.T - P @ G @ P.T)
    gs = 0.5 * (np.diag(P @ np.diag(trM) @ P.T) - np.diag(P @ H @ P.T))
    u = np.asarray(u)
    if bounds is None:
        dls = V._sigmoid(u[o["ls"]])
    else:
        lo, hi = (np.broadcast_to(np.asarray(x, dtype=np.float64), (n_ls,)) for x in bounds)
        sg = V._sigmoid(u[o["ls"]])
        dls = (hi - lo) * sg * (1 - sg)
    g = np.zeros(P_len)
    g[o["mu"]] = -P @ sig
    if independent:
        g[o["scale"]] = np.diag(gB) * V._sigmoid(u[o["scale"]])
    else:
        F = u[o["F"]].reshape(T, 1)
        g[o["F"]] = ((gB + gB.T) @ F).reshape(-1)
        g[o["rv"]] = np.diag(gB) * V._sigmoid(u[o["rv"]])
    g[o["ls"]] = gl * dls
    g[o["noise"]] = gs * V._sigmoid(u[o["noise"]])
    g[o["global"]] = gs.sum() * V._sigmoid(u[o["global"]])
    nt = N * T
    loss = (0.5 * N * np.log(s).sum() + lg + 0.5 * qd) / nt + 0.5 * math.log(2 * math.pi)
    return loss, g / nt


def border_predict(S, u, T, kernel, independent, bounds, isotropic, Xs):
    """mean_t = sum_b k*_{t,b}^T beta_{t,b}, var_t = (complete-grid var_t) + |sum_b Y_{t,b}^T k*_{t,b}|^2, then the T x T mix."""
    (mu, Bm, s, l, ls, lam, Q, P), blocks = R.refl_model(S, u, T, kernel, independent, bounds, isotropic)
    B = S["B"]
    mt, qt = np.zeros((Xs.shape[0], T)), np.zeros((Xs.shape[0], T))
    Ks = []
    for b, (K, dK, w) in enumerate(blocks):
        k, _ = R._refl_cross(S, Xs / ls, ls, kernel, b)
        Ks.append(k * w[:, None] / np.sqrt(B))
    for t in range(T):
        Minv, alpha, Zs, Ls, LS, v, Yb = _task_border(S, blocks, P, mu, lam, t)
        Rm = 0.0
        for b in range(B):
            ks = lam[t] * Ks[b]
            mt[:, t] += ks.T @ (alpha[b] - Yb[b] @ v)
            W = np.linalg.solve(Ls[b], ks)
            qt[:, t] += (W * W).sum(0)
            Rm = Rm + Yb[b].T @ ks
        qt[:, t] -= (Rm * Rm).sum(0)
    vt = lam[None, :] + 1.0 - qt
    return mu[None, :] + np.sqrt(s)[None, :] * (mt @ Q.T), s[None, :] * (vt @ (Q * Q).T)


CASES = [c for c in R.CASES if c[0] != "1d"]      # (a 1-D "grid" is a list of points: nothing to complete)
FRACS = [0.0, 0.1, 0.3]                           # max(1, frac n) missing pixels: M = 1, 10 %, 30 %


@pytest.mark.parametrize("frac", FRACS)
@pytest.mark.parametrize("grid,T,kernel,independent,isotropic,bounded", CASES)
def test_border_loss_grad_equal_dense_autograd(grid, T, kernel, independent, isotropic, bounded, frac):
    X, Y, Xn, Yn, obs = masked(grid, T, frac, seed=5 + int(10 * frac), data_seed=T + len(grid))
    d = X.shape[0]
    S = gprutils.border_blocks_multi(Xn, Yn)
    assert S["n_obs"] == obs.sum() and len(S["miss"]) == (~obs).sum()
    bounds = R._bounds(d, isotropic, bounded)
    dense = V.Dense(X.reshape(d, -1).T[obs], Yn.reshape(-1, T)[obs], kernel, independent, bounds, isotropic)
    n_ls = 1 if isotropic else d
    for k in range(2):
        u = V.random_u(T, n_ls, independent, seed=7 * k + T)
        l0, g0 = dense.loss_grad(u)
        l1, g1 = border_loss_grad(S, u, T, kernel, independent, bounds, isotropic)
        assert abs(l1 - l0) <= 1e-10 * abs(l0), (l1, l0)
        assert np.abs(g1 - g0).max() <= 1e-10 * np.abs(g0).max(), np.abs(g1 - g0).max() / np.abs(g0).max()


@pytest.mark.parametrize("grid,T,kernel,independent,isotropic,bounded", CASES[::2])
def test_border_prediction_equals_dense(grid, T, kernel, independent, isotropic, bounded):
    X, Y, Xn, Yn, obs = masked(grid, T, 1.0 / 6.0, seed=1, data_seed=3 * T)
    d = X.shape[0]
    S = gprutils.border_blocks_multi(Xn, Yn)
    bounds = R._bounds(d, isotropic, bounded)
    u = V.random_u(T, 1 if isotropic else d, independent, seed=T)
    rng = np.random.default_rng(T)
    axes = R.GRIDS[grid]
    lo, hi = np.array([a[0] for a in axes]), np.array([a[-1] for a in axes])
    pts = X.reshape(d, -1).T
    Xs = np.concatenate([rng.uniform(lo - 1, hi + 1, size=(17, d)), pts[:5], pts[~obs][:5]])
    m0, v0 = V.Dense(pts[obs], Yn.reshape(-1, T)[obs], kernel, independent, bounds, isotropic).predict(u, Xs)
    m1, v1 = border_predict(S, u, T, kernel, independent, bounds, isotropic, Xs)
    assert np.abs(m1 - m0).max() <= 1e-10 * np.abs(Y).max()
    assert np.abs(v1 - v0).max() <= 1e-10 * np.abs(v0).max()


@pytest.mark.parametrize("grid", [g for g in R.GRIDS if g != "1d"])
def test_blocks_keep_norms_and_observed_ones(grid):
    T = 3
    X, Y, Xn, Yn, obs = masked(grid, T, 0.25, seed=0, data_seed=1)
    S = gprutils.border_blocks_multi(Xn, Yn)
    B, Nq = S["B"], S["Xq"].shape[0]
    assert S["ys"].shape == (T, B, Nq) and S["ones"].shape == (B, Nq) and S["n_obs"] == obs.sum()
    Yo = Yn.reshape(-1, T)[obs]
    for a in range(T):      # U is orthogonal: sum_b |ys_{a,b}|^2 = |y_a|^2 on the observed rows
        assert abs((S["ys"][a] ** 2).sum() - (Yo[:, a] ** 2).sum()) <= 1e-12 * (Yo[:, a] ** 2).sum()
    # u~^o = U 1_o = U 1 - sum_j coef[:, j] e_{q(j)}  (several missing points can share one representative)
    Xc = np.array(np.meshgrid(*S["axes"], indexing="ij"))
    acc = gprutils.reflection_blocks(Xc, np.ones(Y.shape[:-1]), S["axes"])["ys"].copy()
    for b in range(B):
        np.subtract.at(acc[b], S["q"], S["coef"][b])
    assert np.abs(acc - S["ones"]).max() <= 1e-13
    assert abs((S["ones"] ** 2).sum() - S["n_obs"]) <= 1e-12 * S["n_obs"]
    # the single-output dict underneath is border_blocks' own
    S1 = gprutils.border_blocks(Xn, Yn[..., 0])
    assert np.array_equal(S["q"], S1["q"]) and np.array_equal(S["coef"], S1["coef"]) and np.array_equal(S["miss"], S1["miss"])
    assert np.array_equal(S["ys"][0], S1["ys"])


def test_partial_nan_row_is_missing_for_every_task():
    X, Y, Xn, Yn, obs = masked("6x8", 3, 0.1, seed=2, data_seed=4)
    Yp = Yn.copy().reshape(-1, 3)
    Yp[~obs, 1] = 7.0                   # the row still has a NaN output: dropped for all tasks
    S0, S1 = gprutils.border_blocks_multi(Xn, Yn), gprutils.border_blocks_multi(Xn, Yp.reshape(Yn.shape))
    assert np.array_equal(S0["ys"], S1["ys"]) and np.array_equal(S0["miss"], S1["miss"])


def test_index_without_observation_raises():
    X, Y, _ = R.grid_data("6x8", 3, seed=1)
    Xn, Yn = X.copy(), Y.copy()
    Xn[:, 2, :] = np.nan                # a whole row of the image is missing
    Yn[2, :, :] = np.nan
    with pytest.raises(NotImplementedError):
        gprutils.border_blocks_multi(Xn, Yn)
