"""Host-side checks of the border form of the reflection blocks (gprutils.complete_grid / border_blocks, DESIGN.md
section 11): grid completion, the coefficients of the missing points in the reflection basis, and every identity the HIP
engine rests on, in float64 against a dense restatement of the GP on the observed points."""
import numpy as np
import pytest
import torch

from gpim_amd import gprutils

_F64 = torch.float64


def _brute_basis(shape, dims, fund_shape):
    """U (N, B * Nq) column by column from the group action, independent of reflection_blocks: column (b, p) =
    sum_g chi_b(g) e_{g p}, normalised (zero when the combination vanishes)."""
    N, B = int(np.prod(shape)), 1 << len(dims)
    fund = np.indices(fund_shape).reshape(len(shape), -1).T
    U = np.zeros((N, B * len(fund)))
    for b in range(B):
        for pi, p in enumerate(fund):
            v = np.zeros(N)
            for g in range(B):
                x = list(p)
                for j, k in enumerate(dims):
                    if (g >> j) & 1:
                        x[k] = shape[k] - 1 - x[k]
                chi = -1.0 if bin(g & b).count("1") & 1 else 1.0
                v[np.ravel_multi_index(tuple(x), shape)] += chi
            nv = np.linalg.norm(v)
            if nv > 0:
                U[:, b * len(fund) + pi] = v / nv
    return U


def _kernel(kind, Xa, Xb, var, ls, alpha=None):
    a, b = Xa / ls, Xb / ls
    r2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    if kind == "RBF":
        return var * torch.exp(-0.5 * r2)
    if kind == "Matern52":
        r = (r2 + 1e-12).sqrt()
        return var * (1 + 5 ** 0.5 * r + (5.0 / 3) * r2) * torch.exp(-(5 ** 0.5) * r)
    return var * (1 + (0.5 / alpha) * r2).pow(-alpha)


def _problem(axes, missing, seed=0):
    shape = tuple(len(c) for c in axes)
    rng = np.random.default_rng(seed)
    y = rng.standard_normal(shape)
    Xg = np.array(np.meshgrid(*axes, indexing="ij"))
    Xs, ys = Xg.copy(), y.copy()
    for m in missing:
        Xs[(slice(None),) + m] = np.nan
        ys[m] = np.nan
    return Xg, Xs, ys


CASES = {
    "even_even_M1": ([np.arange(6.0), np.arange(8.0)], [(2, 5)]),
    "odd_even_planes": ([np.arange(5.0), np.arange(8.0)], [(2, 1), (2, 6), (0, 3), (4, 3), (1, 1)]),
    "one_symmetric_axis": ([np.array([0.0, 1.0, 2.5, 4.0, 7.0]), np.arange(6.0)], [(1, 2), (3, 3), (4, 0)]),
    "odd_odd_center": ([np.arange(5.0), np.arange(7.0)], [(2, 3), (0, 0), (4, 6)]),
    "three_d": ([np.arange(4.0), np.arange(3.0), np.arange(4.0)], [(0, 1, 0), (3, 1, 3), (1, 0, 2), (2, 2, 1)]),
}


def _random_missing(shape, frac, seed):
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    flat = rng.choice(n, size=int(round(frac * n)), replace=False)
    return [np.unravel_index(f, shape) for f in flat]


CASES["odd_even_30pct"] = ([np.arange(7.0), np.arange(8.0)], _random_missing((7, 8), 0.3, 3))
CASES["three_d_30pct"] = ([np.arange(5.0), np.arange(4.0), np.arange(3.0)], _random_missing((5, 4, 3), 0.3, 4))


def test_complete_grid_axes_and_missing():
    axes = [np.linspace(-1.0, 2.0, 5), np.arange(6.0) * 0.5]
    Xg, Xs, ys = _problem(axes, [(0, 0), (4, 5), (2, 3)])
    ax, miss = gprutils.complete_grid(Xs, ys)
    assert np.array_equal(ax[0], axes[0]) and np.array_equal(ax[1], axes[1])
    assert miss.tolist() == sorted([0 * 6 + 0, 4 * 6 + 5, 2 * 6 + 3])


def test_complete_grid_rejects():
    axes = [np.arange(4.0), np.arange(5.0)]
    # a whole row missing: its coordinate is unknown
    Xg, Xs, ys = _problem(axes, [(1, j) for j in range(5)])
    with pytest.raises(NotImplementedError):
        gprutils.complete_grid(Xs, ys)
    # not a product grid
    Xg, Xs, ys = _problem(axes, [(0, 0)])
    Xs[1, 2, 3] += 0.25
    with pytest.raises(NotImplementedError):
        gprutils.complete_grid(Xs, ys)
    # NaN patterns of X and y differ
    Xg, Xs, ys = _problem(axes, [(0, 0)])
    ys[1, 1] = np.nan
    with pytest.raises(NotImplementedError):
        gprutils.complete_grid(Xs, ys)


@pytest.mark.parametrize("name", sorted(CASES))
def test_coefficients_against_brute_basis(name):
    axes, missing = CASES[name]
    Xg, Xs, ys = _problem(axes, missing)
    S = gprutils.border_blocks(Xs, ys)
    shape = ys.shape
    fund_shape = tuple((shape[k] + 1) // 2 if k in S["dims"] else shape[k] for k in range(len(shape)))
    U = _brute_basis(shape, S["dims"], fund_shape)
    Nq = S["Xq"].shape[0]
    # the projected observations (y = 0 at the missing points) and the coefficients of the missing points
    yt = np.nan_to_num(ys, nan=0.0).ravel()
    assert np.allclose((U.T @ yt).reshape(S["B"], Nq), S["ys"], atol=1e-12)
    assert len(S["miss"]) == len(missing) and S["n_obs"] == ys.size - len(missing)
    for j, f in enumerate(S["miss"]):
        col = (U.T[:, f]).reshape(S["B"], Nq)
        expect = np.zeros_like(col)
        expect[:, S["q"][j]] = S["coef"][:, j]
        assert np.allclose(col, expect, atol=1e-12), (name, j)
    # the complete grid gives what reflection_blocks gives, and it was not changed
    R = gprutils.reflection_blocks(Xg, np.nan_to_num(ys, nan=0.0), gprutils.complete_grid(Xs, ys)[0])
    assert R["mask"] == S["mask"] and R["B"] == S["B"] and np.array_equal(R["Xq"], S["Xq"])
    assert np.array_equal(R["ys"], S["ys"])


def _blocks_torch(kind, S, Xg, var, ls, noise, alpha, jitter):
    """B_b = U_b^T A U_b from the brute-force basis (identity rows where a point does not exist in a block)."""
    shape = Xg.shape[1:]
    fund_shape = tuple((shape[k] + 1) // 2 if k in S["dims"] else shape[k] for k in range(len(shape)))
    U = torch.from_numpy(_brute_basis(shape, S["dims"], fund_shape))
    Xf = torch.from_numpy(Xg.reshape(Xg.shape[0], -1).T.copy())
    A = _kernel(kind, Xf, Xf, var, ls, alpha) + (noise + jitter) * torch.eye(Xf.shape[0], dtype=_F64)
    Nq = S["Xq"].shape[0]
    blocks = []
    for b in range(S["B"]):
        Ub = U[:, b * Nq:(b + 1) * Nq]
        Bb = Ub.T @ A @ Ub
        absent = (Ub.abs().sum(0) == 0)
        Bb = Bb + torch.diag(absent.to(_F64))
        blocks.append(Bb)
    return A, U, blocks


@pytest.mark.parametrize("kind", ["RBF", "Matern52", "RationalQuadratic"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_border_identities(name, kind):
    axes, missing = CASES[name]
    Xg, Xs, ys = _problem(axes, missing, seed=1)
    S = gprutils.border_blocks(Xs, ys)
    B, Nq, M = S["B"], S["Xq"].shape[0], len(S["miss"])
    q, coef = torch.from_numpy(S["q"].astype(np.int64)), torch.from_numpy(S["coef"])
    jitter = 1e-5
    ls = torch.tensor([1.3, 2.1, 1.7][:Xg.shape[0]], dtype=_F64, requires_grad=True)
    var = torch.tensor(0.8, dtype=_F64, requires_grad=True)
    noise = torch.tensor(0.05, dtype=_F64, requires_grad=True)
    alpha = torch.tensor(1.5, dtype=_F64, requires_grad=True)
    A, U, blocks = _blocks_torch(kind, S, Xg, var, ls, noise, alpha, jitter)
    obs = torch.from_numpy(np.setdiff1d(np.arange(ys.size), S["miss"]))
    y_o = torch.from_numpy(ys.ravel()[obs.numpy()])
    A_oo = A[obs][:, obs]
    # dense restatement: the GP on the observed points
    L_oo = torch.linalg.cholesky(A_oo)
    a_o = torch.cholesky_solve(y_o[:, None], L_oo)[:, 0]
    quad_d = (y_o * a_o).sum()
    logdet_d = 2 * torch.log(torch.diagonal(L_oo)).sum()
    nll_d = 0.5 * quad_d + 0.5 * logdet_d
    g_dense = torch.autograd.grad(nll_d, [var, ls, noise, alpha], allow_unused=True)
    with torch.no_grad():
        Binv = [torch.linalg.inv(Bb) for Bb in blocks]
        ysb = torch.from_numpy(S["ys"])
        al = [Binv[b] @ ysb[b] for b in range(B)]
        # S = (A^-1)_mm from the blocks, against the dense inverse
        Smat = sum(coef[b][:, None] * coef[b][None, :] * Binv[b][q][:, q] for b in range(B))
        Ainv = torch.linalg.inv(A.detach())
        miss = torch.from_numpy(S["miss"])
        assert torch.allclose(Smat, Ainv[miss][:, miss], rtol=0, atol=1e-10 * Ainv.abs().max())
        LS = torch.linalg.cholesky(Smat)
        LSi = torch.linalg.inv(LS)
        # log det A_oo = log det A + log det S
        logdet_b = sum(torch.linalg.slogdet(Bb)[1] for Bb in blocks) + 2 * torch.log(torch.diagonal(LS)).sum()
        assert abs(logdet_b - logdet_d) <= 1e-10 * max(1.0, abs(logdet_d))
        # quadratic form: y~^T A^-1 y~ - |L_S^-1 t|^2, t = (A^-1 y~)_m
        t = sum(coef[b] * al[b][q] for b in range(B))
        v = LSi @ t
        quad_b = sum((ysb[b] * al[b]).sum() for b in range(B)) - (v * v).sum()
        assert abs(quad_b - quad_d) <= 1e-10 * max(1.0, abs(quad_d))
        # Y_b = C_b L_S^-T, C_b[:, j] = c_b(j) B_b^-1[:, q(j)];  a_b = alpha_b - Y_b L_S^-1 t = (U^T alpha)_b
        Y = [(Binv[b][:, q] * coef[b][None, :]) @ LSi.T for b in range(B)]
        a = [al[b] - Y[b] @ v for b in range(B)]
        alpha_full = torch.zeros(ys.size, dtype=_F64)
        alpha_full[obs] = a_o
        Ua = (U.T @ alpha_full).reshape(B, Nq)
        for b in range(B):
            assert torch.allclose(a[b], Ua[b], rtol=0, atol=1e-10 * max(1.0, Ua.abs().max().item()))
        G = [Binv[b] - Y[b] @ Y[b].T - torch.outer(a[b], a[b]) for b in range(B)]
    # gradient: 0.5 sum_b <G_b, dB_b> equals the dense gradient (points absent from a block contribute nothing)
    A2, _, blocks2 = _blocks_torch(kind, S, Xg, var, ls, noise, alpha, jitter)
    contr = 0.5 * sum((G[b] * blocks2[b]).sum() for b in range(B))
    g_border = torch.autograd.grad(contr, [var, ls, noise, alpha], allow_unused=True)
    for gd, gb in zip(g_dense, g_border):
        if gd is None:
            assert gb is None or torch.all(gb == 0)
            continue
        assert torch.allclose(gb, gd, rtol=1e-10, atol=1e-10 * max(1.0, gd.abs().max().item())), (gb, gd)
    with torch.no_grad():
        # posterior variance at test points (a finer grid): complete-grid variance + |sum_b Y_b^T k*_b|^2
        Xt = torch.from_numpy(np.array(np.meshgrid(*[np.linspace(c[0], c[-1], 3) for c in axes],
                                                   indexing="ij")).reshape(len(axes), -1).T.copy())
        Xf = torch.from_numpy(Xg.reshape(Xg.shape[0], -1).T.copy())
        Ks = _kernel(kind, Xf, Xt, var, ls, alpha)
        Kss = var * torch.ones(Xt.shape[0], dtype=_F64)
        ksb = (U.T @ Ks).reshape(B, Nq, -1)
        var_full = Kss - sum((ksb[b] * (Binv[b] @ ksb[b])).sum(0) for b in range(B))
        R = sum(Y[b].T @ ksb[b] for b in range(B))
        var_b = var_full + (R * R).sum(0)
        Ko = Ks[obs]
        var_d = Kss - (Ko * torch.cholesky_solve(Ko, L_oo)).sum(0)
        assert torch.allclose(var_b, var_d, rtol=0, atol=1e-10)
        mean_b = sum(ksb[b].T @ a[b] for b in range(B))
        mean_d = Ko.T @ a_o
        assert torch.allclose(mean_b, mean_d, rtol=0, atol=1e-10)


def test_border_flops_choice():
    # a 256 x 256 image with 10 % missing: the border is cheaper; the spiral twin (74 % missing): dense
    fb, fd = gprutils.border_flops(65536, 6554, 2)
    assert fb < 0.5 * fd
    fb, fd = gprutils.border_flops(16384, 12170, 2)
    assert fb > 0.5 * fd
