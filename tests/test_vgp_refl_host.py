"""CPU checks of the multi-output GP's reflection solver (vreconstructor on complete grids): the loss,
gradient, predictive mean and variance restated from gprutils.reflection_blocks_multi -- T 2^r blocks lambda_t K_b + I of
N_q points -- against the dense N T x N T restatement of tests/vgp_oracle.py (autograd)."""
import math

import numpy as np
import pytest

import vgp_oracle as V
from gpim_amd import gprutils


def _kernel(r2, kernel):
    """k(r2) and h = -2 dk/dr2 (the lengthscale derivative factor of vgp_oracle._kmat_np)."""
    if kernel == "RBF":
        k = np.exp(-0.5 * r2)
        return k, k
    r = np.sqrt(r2 + 1e-12)
    ex = np.exp(-V.SQRT5 * r)
    return (1.0 + V.SQRT5 * r + (5.0 / 3.0) * r2) * ex, (5.0 / 3.0) * (1.0 + V.SQRT5 * (r2 / r)) * ex


def _refl_cross(S, Za, ls, kernel, b, grad=False):
    """sum_g chi_b(g) k(p, g z) for p in the domain (rows) and z in Za (columns, already scaled by 1 / l), and the
    lengthscale derivative factors sum_g chi_b(g) h (scaled difference_k)^2 / l_k."""
    d = S["Xq"].shape[1]
    a = S["Xq"] / ls
    cz = np.asarray(S["twoc"][:d]) / ls
    dims = S["dims"]
    K = np.zeros((a.shape[0], Za.shape[0]))
    dK = [np.zeros_like(K) for _ in range(d)]
    for g in range(1 << len(dims)):
        refl = {dims[j] for j in range(len(dims)) if (g >> j) & 1}
        diff = [(a[:, k][:, None] + Za[:, k][None, :] - cz[k]) if k in refl else (a[:, k][:, None] - Za[:, k][None, :])
                for k in range(d)]
        r2 = sum(x * x for x in diff)
        k, h = _kernel(r2, kernel)
        chi = -1.0 if bin(g & b).count("1") & 1 else 1.0
        K += chi * k
        if grad:
            for q in range(d):
                dK[q] += chi * h * diff[q] ** 2 / ls[q]
    return K, dK


def refl_model(S, u, T, kernel, independent, bounds, isotropic):
    """Per-task/block quantities of the reflected model at u: (params, blocks) with blocks[t][b] = (A, L, beta, K_b, dK_b)."""
    d = S["Xq"].shape[1]
    n_ls = 1 if isotropic else d
    mu, Bm, s, l = (t.numpy() for t in V.params_torch(__import__("torch").as_tensor(u), T, n_ls, independent,
                                                        None if bounds is None else bounds))
    ls = np.broadcast_to(l, (d,)).copy()
    lam, Q = np.linalg.eigh(Bm / np.sqrt(np.outer(s, s)))
    P = Q / np.sqrt(s)[:, None]
    B, Nq = S["B"], S["Xq"].shape[0]
    blocks = []
    for b in range(B):
        K, dK = _refl_cross(S, S["Xq"] / ls, ls, kernel, b, grad=True)
        w = np.ones(Nq) if S["wts"] is None else S["wts"][b]
        W = np.outer(w, w)
        K, dK = K * W, [x * W for x in dK]
        if isotropic:
            dK = [sum(dK)]
        blocks.append((K, dK, w))
    return (mu, Bm, s, l, ls, lam, Q, P), blocks


def refl_loss_grad(S, u, T, kernel, independent, bounds, isotropic):
    """section 9's loss and gradient with every task's quantities summed over its 2^r blocks."""
    d = S["Xq"].shape[1]
    n_ls = 1 if isotropic else d
    o, P_len = V.layout(T, n_ls, independent)
    (mu, Bm, s, l, ls, lam, Q, P), blocks = refl_model(S, u, T, kernel, independent, bounds, isotropic)
    B, N = S["B"], S["n_total"]
    lg = q = 0.0
    trMK, trM = np.zeros(T), np.zeros(T)
    gl = np.zeros(n_ls)
    H, G, sig = np.zeros((T, T)), np.zeros((T, T)), np.zeros(T)
    for b, (K, dK, w) in enumerate(blocks):
        present = w != 0
        Z = np.einsum("at,ai->ti", P, S["ys"][:, b] - mu[:, None] * S["ones"][b][None, :])
        Z[:, ~present] = 0.0
        beta = np.empty_like(Z)
        for t in range(T):
            A = lam[t] * K + np.eye(K.shape[0])
            A[~present, :] = 0.0
            A[:, ~present] = 0.0
            A[~present, ~present] = 1.0                   # absent points: identity rows
            L = np.linalg.cholesky(A)
            M = np.linalg.inv(A)
            beta[t] = M @ Z[t]
            lg += np.log(np.diag(L)).sum()
            q += Z[t] @ beta[t]
            trMK[t] += (M * K).sum()
            trM[t] += np.trace(M[np.ix_(present, present)])
            for k in range(n_ls):
                gl[k] += 0.5 * lam[t] * ((M * dK[k]).sum() - beta[t] @ dK[k] @ beta[t])
        H += beta @ beta.T
        G += beta @ K @ beta.T
        sig += beta @ S["ones"][b]
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
    loss = (0.5 * N * np.log(s).sum() + lg + 0.5 * q) / nt + 0.5 * math.log(2 * math.pi)
    return loss, g / nt


def refl_predict(S, u, T, kernel, independent, bounds, isotropic, Xs):
    """mean_t = sum_b k*_{t,b}^T beta_{t,b}, var_t = lambda_t + 1 - sum_b |L_{t,b}^-1 k*_{t,b}|^2 (K* scale B^-1/2), then the
    T x T mix of vgp_combine_kernel; M x T each."""
    (mu, Bm, s, l, ls, lam, Q, P), blocks = refl_model(S, u, T, kernel, independent, bounds, isotropic)
    B = S["B"]
    mt, qt = np.zeros((Xs.shape[0], T)), np.zeros((Xs.shape[0], T))
    for b, (K, dK, w) in enumerate(blocks):
        present = w != 0
        Ks, _ = _refl_cross(S, Xs / ls, ls, kernel, b)
        Ks *= w[:, None] / np.sqrt(B)
        Z = np.einsum("at,ai->ti", P, S["ys"][:, b] - mu[:, None] * S["ones"][b][None, :])
        Z[:, ~present] = 0.0
        for t in range(T):
            A = lam[t] * K + np.eye(K.shape[0])
            A[~present, :] = 0.0
            A[:, ~present] = 0.0
            A[~present, ~present] = 1.0
            L = np.linalg.cholesky(A)
            ks = lam[t] * Ks
            mt[:, t] += ks.T @ np.linalg.solve(A, Z[t])
            W = np.linalg.solve(L, ks)
            qt[:, t] += (W * W).sum(0)
    vt = lam[None, :] + 1.0 - qt
    mean = mu[None, :] + np.sqrt(s)[None, :] * (mt @ Q.T)
    var = s[None, :] * (vt @ (Q * Q).T)
    return mean, var


GRIDS = {   # name: the axis coordinate vectors
    "1d": [np.arange(9.0)],
    "6x8": [np.arange(6.0), np.arange(8.0)],
    "7x6": [np.arange(7.0), 0.5 * np.arange(6.0)],
    "5x5": [np.arange(5.0), np.arange(5.0)],
    "4x3x5": [np.arange(4.0), np.arange(3.0), 0.8 * np.arange(5.0)],
    "nonsym": [np.array([0.0, 1.0, 2.0, 4.0, 4.5]), np.arange(6.0)],      # axis 0 not symmetric: only axis 1 is reflected
}


def grid_data(name, T, seed):
    axes = GRIDS[name]
    X = np.array(np.meshgrid(*axes, indexing="ij"))
    rng = np.random.default_rng(seed)
    pts = X.reshape(X.shape[0], -1).T
    base = np.stack([np.sin(pts @ rng.normal(size=pts.shape[1]) * 0.6 + rng.uniform(0, 6)) for _ in range(3)], 1)
    Y = base @ rng.normal(size=(3, T)) + 0.1 * rng.normal(size=(pts.shape[0], T)) + rng.normal(size=T)
    return X, Y.reshape(X.shape[1:] + (T,)), axes


CASES = [  # grid, T, kernel, independent, isotropic, bounded
    ("1d", 3, "RBF", False, False, True),
    ("6x8", 1, "Matern52", False, False, True),
    ("6x8", 5, "RBF", True, True, False),
    ("7x6", 3, "Matern52", False, False, False),
    ("7x6", 5, "Matern52", True, False, True),
    ("5x5", 3, "RBF", False, True, True),
    ("5x5", 1, "Matern52", True, False, False),
    ("4x3x5", 3, "Matern52", False, False, True),
    ("4x3x5", 1, "RBF", True, True, False),
    ("nonsym", 3, "RBF", False, False, True),
    ("nonsym", 5, "Matern52", True, True, False),
]


def _bounds(d, isotropic, bounded):
    if not bounded:
        return None
    return (0.5, 2.5) if isotropic else ([0.5] * d, [2.5 + 0.5 * k for k in range(d)])


@pytest.mark.parametrize("grid,T,kernel,independent,isotropic,bounded", CASES)
def test_reflected_loss_grad_equal_dense_autograd(grid, T, kernel, independent, isotropic, bounded):
    X, Y, axes = grid_data(grid, T, seed=T + len(grid))
    d = X.shape[0]
    S = gprutils.reflection_blocks_multi(X, Y, axes)
    if grid == "nonsym":
        assert S["dims"] == [1]
    bounds = _bounds(d, isotropic, bounded)
    dense = V.Dense(X.reshape(d, -1).T, Y.reshape(-1, T), kernel, independent, bounds, isotropic)
    n_ls = 1 if isotropic else d
    for k in range(2):
        u = V.random_u(T, n_ls, independent, seed=7 * k + T)
        l0, g0 = dense.loss_grad(u)
        l1, g1 = refl_loss_grad(S, u, T, kernel, independent, bounds, isotropic)
        assert abs(l1 - l0) <= 1e-10 * abs(l0), (l1, l0)
        assert np.abs(g1 - g0).max() <= 1e-10 * np.abs(g0).max(), np.abs(g1 - g0).max() / np.abs(g0).max()


@pytest.mark.parametrize("grid,T,kernel,independent,isotropic,bounded", CASES[::2])
def test_reflected_prediction_equals_dense(grid, T, kernel, independent, isotropic, bounded):
    X, Y, axes = grid_data(grid, T, seed=3 * T)
    d = X.shape[0]
    S = gprutils.reflection_blocks_multi(X, Y, axes)
    bounds = _bounds(d, isotropic, bounded)
    u = V.random_u(T, 1 if isotropic else d, independent, seed=T)
    rng = np.random.default_rng(T)
    lo, hi = np.array([a[0] for a in axes]), np.array([a[-1] for a in axes])
    Xs = np.concatenate([rng.uniform(lo - 1, hi + 1, size=(17, d)), X.reshape(d, -1).T[:5]])
    m0, v0 = V.Dense(X.reshape(d, -1).T, Y.reshape(-1, T), kernel, independent, bounds, isotropic).predict(u, Xs)
    m1, v1 = refl_predict(S, u, T, kernel, independent, bounds, isotropic, Xs)
    scale = np.abs(Y).max()
    assert np.abs(m1 - m0).max() <= 1e-10 * scale
    assert np.abs(v1 - v0).max() <= 1e-10 * np.abs(v0).max()


@pytest.mark.parametrize("grid", list(GRIDS))
def test_blocks_keep_norms_and_ones(grid):
    T = 3
    X, Y, axes = grid_data(grid, T, seed=1)
    S = gprutils.reflection_blocks_multi(X, Y, axes)
    B, Nq = S["B"], S["Xq"].shape[0]
    assert S["ys"].shape == (T, B, Nq) and S["ones"].shape == (B, Nq)
    for a in range(T):      # U is orthogonal: sum_b |ys_{a,b}|^2 = |y_a|^2, and each task's blocks are reflection_blocks'
        assert abs((S["ys"][a] ** 2).sum() - (Y[..., a] ** 2).sum()) <= 1e-12 * (Y[..., a] ** 2).sum()
        assert np.array_equal(S["ys"][a], gprutils.reflection_blocks(X, Y[..., a], axes)["ys"])
    w0 = np.ones(Nq) if S["wts"] is None else S["wts"][0]
    assert np.allclose(S["ones"][0], np.sqrt(B) * w0, rtol=0, atol=1e-14)
    assert np.abs(S["ones"][1:]).max(initial=0.0) <= 1e-14
    assert abs((S["ones"] ** 2).sum() - Y[..., 0].size) <= 1e-12 * Y[..., 0].size
