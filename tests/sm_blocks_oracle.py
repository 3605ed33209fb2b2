"""Float64 torch restatement of the spectral-mixture GP in the reflection basis of a grid, independent
of the engine: the blocks K_s of gprutils.reflection_blocks* / border_blocks* written out entry by entry (cos of the
difference and of the mirror term a + b - 2 c directly, no angle addition), torch.linalg.cholesky per block, the border
identities of section 11, and the closed-form gradient the engine contracts.  The dense model of the same data is
tests/sm_oracle.py; the two are compared in tests/test_sm_blocks_host.py.

A blocks dict S needs: mask, twoc, dims, B, Xq, ys (B, Nq), ones (B, Nq), wts (B, Nq) or None, n_total, and with a border
q, coef, n_obs."""
import math

import numpy as np
import torch

import sm_oracle as SO

F64 = torch.float64


def block_signs(S, b):
    """sigma_d of block b per data dimension: +-1 on a reflected axis (bit j of b: the j-th reflected axis is odd), 0 else."""
    d = S["Xq"].shape[1]
    sig = [0.0] * d
    for j, k in enumerate(S["dims"]):
        sig[k] = -1.0 if (b >> j) & 1 else 1.0
    return sig


def axis_terms(A, Z, mq, sq, S, b):
    """Per data dimension k the n x m factor F_k = f(a - z) + sigma f(a + z - 2 c), f(t) = exp(-2 pi^2 t^2 s^2) cos(2 pi t m),
    and its derivative parts dF_k / dm = -2 pi (.) and dF_k / ds = -4 pi^2 s (.): three lists of d matrices."""
    sig = block_signs(S, b)
    F, Fm, Fs = [], [], []
    for k in range(A.shape[1]):
        parts = [(A[:, None, k] - Z[None, :, k], 1.0)]
        if sig[k] != 0.0:
            parts.append((A[:, None, k] + Z[None, :, k] - S["twoc"][k], sig[k]))
        f = fm = fs = 0.0
        for t, sg in parts:
            E = sg * torch.exp(-2.0 * math.pi ** 2 * t ** 2 * sq[k] ** 2)
            co, si = torch.cos(2.0 * math.pi * t * mq[k]), torch.sin(2.0 * math.pi * t * mq[k])
            f = f + E * co
            fm = fm + t * si * E
            fs = fs + t ** 2 * E * co
        F.append(f)
        Fm.append(fm)
        Fs.append(fs)
    return F, Fm, Fs


def _weights(S, b):
    n = S["Xq"].shape[0]
    return torch.ones(n, dtype=F64) if S["wts"] is None else torch.as_tensor(S["wts"][b], dtype=F64)


def _expand(v, d, D):
    return v.expand(d) if D == 1 else v


def block_kmat(S, b, u, Q, D, Z=None):
    """K_s of block b at u.  Z None: the Nq x Nq block with the noise on the diagonal of the present points and identity
    rows for the absent ones; else K_s(Xq, Z) with the 1 / sqrt(B) scale of a test point's column.  Keeps u's graph."""
    u = torch.as_tensor(u, dtype=F64)
    A = torch.as_tensor(S["Xq"], dtype=F64)
    sym = Z is None
    Zt = A if sym else torch.as_tensor(Z, dtype=F64)
    d = A.shape[1]
    _, w, m, s, noise = SO.split(u, Q, D)
    K = torch.zeros((A.shape[0], Zt.shape[0]), dtype=F64)
    for q in range(Q):
        F, _, _ = axis_terms(A, Zt, _expand(m[q], d, D), _expand(s[q], d, D), S, b)
        P = F[0]
        for k in range(1, d):
            P = P * F[k]
        K = K + w[q] * P
    wr = _weights(S, b)
    if not sym:
        return K * wr[:, None] / math.sqrt(S["B"])
    present = wr != 0
    K = K * wr[:, None] * wr[None, :] + torch.diag(torch.where(present, noise, torch.ones((), dtype=F64)))
    return K


def _state(S, u, Q, D):
    """Per block: K_s^-1 and alpha_s of r_s = ys_s - c ones_s, corrected by the border when S has one; the quadratic form and
    sum log diag of the whole model."""
    u = torch.as_tensor(u, dtype=F64)
    B = S["B"]
    c = u[0]
    ys, ones = torch.as_tensor(S["ys"], dtype=F64), torch.as_tensor(S["ones"], dtype=F64)
    Binv, alpha = [], []
    q2, lg = 0.0, 0.0
    for b in range(B):
        L = torch.linalg.cholesky(block_kmat(S, b, u, Q, D))
        r = (ys[b] - c * ones[b])[:, None]
        z = torch.linalg.solve_triangular(L, r, upper=False)
        q2 = q2 + (z ** 2).sum()
        lg = lg + torch.log(torch.diagonal(L)).sum()
        Binv.append(torch.cholesky_inverse(L))
        alpha.append(torch.cholesky_solve(r, L)[:, 0])
    if "q" in S and len(S["q"]):
        qi = torch.as_tensor(np.asarray(S["q"], dtype=np.int64))
        coef = torch.as_tensor(S["coef"], dtype=F64)
        Sm = sum(torch.outer(coef[b], coef[b]) * Binv[b][qi][:, qi] for b in range(B))
        t = sum(coef[b] * alpha[b][qi] for b in range(B))
        Ls = torch.linalg.cholesky(Sm)
        v = torch.linalg.solve_triangular(Ls, t[:, None], upper=False)
        q2 = q2 - (v ** 2).sum()
        lg = lg + torch.log(torch.diagonal(Ls)).sum()
        for b in range(B):
            C = Binv[b][:, qi] * coef[b][None, :]
            Y = torch.linalg.solve_triangular(Ls, C.T, upper=False).T           # C L_S^-T
            alpha[b] = alpha[b] - (Y @ v)[:, 0]
            Binv[b] = Binv[b] - Y @ Y.T
    return Binv, alpha, q2, lg


def n_points(S):
    return S["n_obs"] if "n_obs" in S else S["n_total"]


def loss(S, u, Q, D):
    """The dense model's loss from the blocks (torch scalar, keeps u's graph)."""
    _, _, q2, lg = _state(S, u, Q, D)
    return (0.5 * q2 + lg) / n_points(S) + 0.5 * math.log(2 * math.pi)


def closed_grad(S, u, Q, D):
    """The gradient the engine forms: G_s = K_s^-1 - alpha_s alpha_s^T contracted with dK_s / dtheta block by block (the
    derivative of a product of per-axis sums replaces one axis's factor), tr G over the present points, c through
    ones_s^T alpha_s."""
    ut = torch.as_tensor(np.asarray(u, dtype=np.float64))
    with torch.no_grad():
        Binv, alpha, _, _ = _state(S, ut, Q, D)
        A = torch.as_tensor(S["Xq"], dtype=F64)
        d = A.shape[1]
        n = n_points(S)
        _, w, m, s, _ = SO.split(ut, Q, D)
        ones = torch.as_tensor(S["ones"], dtype=F64)
        g = torch.zeros(ut.numel(), dtype=F64)
        dsp = torch.sigmoid(ut)
        h = 0.5 / n
        for b in range(S["B"]):
            wr = _weights(S, b)
            G = (Binv[b] - torch.outer(alpha[b], alpha[b])) * wr[:, None] * wr[None, :]
            g[0] -= (ones[b] * alpha[b]).sum() / n
            g[-1] += h * torch.diagonal(Binv[b] - torch.outer(alpha[b], alpha[b]))[wr != 0].sum() * dsp[-1]
            for q in range(Q):
                sq = _expand(s[q], d, D)
                F, Fm, Fs = axis_terms(A, A, _expand(m[q], d, D), sq, S, b)
                P = torch.ones_like(G)
                for k in range(d):
                    P = P * F[k]
                g[1 + q] += h * (G * P).sum() * dsp[1 + q]
                gm, gs = torch.zeros(d, dtype=F64), torch.zeros(d, dtype=F64)
                for k in range(d):
                    oth = torch.ones_like(G)
                    for e in range(d):
                        if e != k:
                            oth = oth * F[e]
                    gm[k] = h * (G * (-2.0 * math.pi * w[q]) * Fm[k] * oth).sum()
                    gs[k] = h * (G * (-4.0 * math.pi ** 2 * sq[k] * w[q]) * Fs[k] * oth).sum()
                if D == 1:
                    gm, gs = gm.sum().reshape(1), gs.sum().reshape(1)
                im = 1 + Q + q * D
                isx = 1 + Q + Q * D + q * D
                g[im:im + D] += gm * dsp[im:im + D]
                g[isx:isx + D] += gs * dsp[isx:isx + D]
    return g.numpy()


def grid(shape, axes=None):
    axes = [np.arange(n, dtype=np.float64) for n in shape] if axes is None else axes
    return np.array(np.meshgrid(*axes, indexing="ij"))


def with_holes(X, y):
    X = X.copy()
    X[:, np.isnan(y)] = np.nan
    return X


def blocks_of(X, y):
    """The blocks dict of a single-output model: gprutils' multi-output helpers with one task (ys, and ones = U 1 / U 1_o)."""
    from gpim_amd import gprutils as U
    if np.isnan(y).any():
        B = U.border_blocks_multi(X, y[..., None])
    else:
        B = U.reflection_blocks_multi(X, y[..., None], U.grid_axes(X)[0])
    B["ys"] = B["ys"][0]
    return B


def flat(X, y):
    from gpim_amd import gprutils as U
    Xt, yt = U.prepare_training_data(X, y)
    return Xt.numpy(), yt.numpy()


def smooth_image(shape, seed):
    """A quasi-periodic image of the given shape with a little noise (float64)."""
    rng = np.random.default_rng(seed)
    idx = np.indices(shape).astype(np.float64)
    y = np.ones(shape)
    for k in range(len(shape)):
        y = y * np.cos(2 * np.pi * idx[k] / (5.0 + 2.0 * k) + 0.3 * k)
    return y + 0.4 + 0.05 * rng.normal(size=shape)


def punch(y, n_missing, seed, forced=()):
    """y with n_missing NaN entries: the flat indices in ``forced`` first, the rest drawn at random."""
    rng = np.random.default_rng(seed)
    y = y.copy()
    flat = list(forced)
    rest = [i for i in rng.permutation(y.size) if i not in set(flat)]
    flat += rest[:n_missing - len(flat)]
    y.reshape(-1)[np.asarray(flat, dtype=np.int64)] = np.nan
    return y
