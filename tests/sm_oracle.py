"""Dense float64 torch restatement of the spectral-mixture GP of skreconstructor(kernel='Spectral') (GPyTorch semantics;
include/gpimhip.h: gpimhip_fit_sm), independent of gpim_amd: the covariance as GPyTorch's SpectralMixtureKernel.forward
writes it (cos of the difference, no angle addition), torch.linalg.cholesky, autograd, torch.optim.Adam over the raw
vector u = [c | r_w (Q) | r_m (Q x D) | r_s (Q x D) | r_n], and the analytic predictive."""
import math

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64


def split(u, Q, D):
    c = u[0]
    w = F.softplus(u[1:1 + Q])
    m = F.softplus(u[1 + Q:1 + Q + Q * D]).reshape(Q, D)
    s = F.softplus(u[1 + Q + Q * D:1 + Q + 2 * Q * D]).reshape(Q, D)
    noise = 1e-4 + F.softplus(u[1 + Q + 2 * Q * D])
    return c, w, m, s, noise


def kmat(X, Z, u, Q, D):
    """sum_q w_q exp(-2 pi^2 sum_d tau_d^2 s_qd^2) prod_d cos(2 pi tau_d m_qd), tau = x - z; (N, M)."""
    X, Z = torch.as_tensor(X, dtype=F64), torch.as_tensor(Z, dtype=F64)
    u = torch.as_tensor(u, dtype=F64)
    _, w, m, s, _ = split(u, Q, D)
    tau = X[:, None, :] - Z[None, :, :]                       # N x M x d
    d = X.shape[1]
    K = torch.zeros(tau.shape[:2], dtype=F64)
    for q in range(Q):
        mq = m[q].expand(d) if D == 1 else m[q]
        sq = s[q].expand(d) if D == 1 else s[q]
        e = torch.exp(-2.0 * math.pi ** 2 * (tau ** 2 * sq ** 2).sum(-1))
        cpart = torch.cos(2.0 * math.pi * tau * mq).prod(-1)
        K = K + w[q] * e * cpart
    return K


def loss(u, X, y, Q, D):
    """-log N(y | c, K + noise I) / N  (ExactMarginalLogLikelihood, negated); u: torch tensor (autograd-friendly)."""
    X = torch.as_tensor(X, dtype=F64)
    y = torch.as_tensor(y, dtype=F64)
    N = X.shape[0]
    c, _, _, _, noise = split(u, Q, D)
    K = kmat_t(X, u, Q, D) + noise * torch.eye(N, dtype=F64)
    L = torch.linalg.cholesky(K)
    r = (y - c)[:, None]
    z = torch.linalg.solve_triangular(L, r, upper=False)
    return (0.5 * (z ** 2).sum() + torch.log(torch.diagonal(L)).sum() + 0.5 * N * math.log(2 * math.pi)) / N


def kmat_t(X, u, Q, D):
    """kmat(X, X) keeping u's autograd graph."""
    _, w, m, s, _ = split(u, Q, D)
    tau = X[:, None, :] - X[None, :, :]
    d = X.shape[1]
    K = torch.zeros(tau.shape[:2], dtype=F64)
    for q in range(Q):
        mq = m[q].expand(d) if D == 1 else m[q]
        sq = s[q].expand(d) if D == 1 else s[q]
        K = K + w[q] * torch.exp(-2.0 * math.pi ** 2 * (tau ** 2 * sq ** 2).sum(-1)) * torch.cos(2.0 * math.pi * tau * mq).prod(-1)
    return K


def loss_grad(u, X, y, Q, D):
    """(loss, d loss / du) by autograd; numpy in, float / numpy out."""
    ut = torch.tensor(np.asarray(u, dtype=np.float64), requires_grad=True)
    val = loss(ut, X, y, Q, D)
    val.backward()
    return float(val.item()), ut.grad.numpy().copy()


def closed_grad(u, X, y, Q, D):
    """The closed-form gradient of the engine (include/gpimhip.h, csrc/sm.hip): G = K^-1 - alpha alpha^T,
    d loss / d theta = (1/2N) sum_ij G_ij dK_ij / d theta; c through sum alpha, noise through tr G."""
    X = torch.as_tensor(X, dtype=F64)
    y = torch.as_tensor(y, dtype=F64)
    ut = torch.as_tensor(np.asarray(u, dtype=np.float64))
    N, d = X.shape
    c, w, m, s, noise = split(ut, Q, D)
    K = kmat_t(X, ut, Q, D) + noise * torch.eye(N, dtype=F64)
    Kinv = torch.cholesky_inverse(torch.linalg.cholesky(K))
    alpha = Kinv @ (y - c)
    G = Kinv - torch.outer(alpha, alpha)
    tau = X[:, None, :] - X[None, :, :]
    g = torch.zeros(ut.numel(), dtype=F64)
    g[0] = -alpha.sum() / N
    h = 0.5 / N
    dsp = torch.sigmoid(ut)
    for q in range(Q):
        mq = m[q].expand(d) if D == 1 else m[q]
        sq = s[q].expand(d) if D == 1 else s[q]
        E = torch.exp(-2.0 * math.pi ** 2 * (tau ** 2 * sq ** 2).sum(-1))
        cos = torch.cos(2.0 * math.pi * tau * mq)
        sin = torch.sin(2.0 * math.pi * tau * mq)
        kq = E * cos.prod(-1)
        g[1 + q] = h * (G * kq).sum() * dsp[1 + q]
        gm = torch.zeros(d, dtype=F64)
        gs = torch.zeros(d, dtype=F64)
        for k in range(d):
            oth = torch.ones_like(E)
            for e in range(d):
                if e != k:
                    oth = oth * cos[..., e]
            dm = -2.0 * math.pi * tau[..., k] * sin[..., k] * w[q] * E * oth
            ds = -4.0 * math.pi ** 2 * tau[..., k] ** 2 * sq[k] * w[q] * kq
            gm[k] = h * (G * dm).sum()
            gs[k] = h * (G * ds).sum()
        if D == 1:
            gm, gs = gm.sum().reshape(1), gs.sum().reshape(1)
        im = 1 + Q + q * D
        isx = 1 + Q + Q * D + q * D
        g[im:im + D] = gm * dsp[im:im + D]
        g[isx:isx + D] = gs * dsp[isx:isx + D]
    g[-1] = h * torch.diagonal(G).sum() * dsp[-1]
    return g.numpy()


def initial_raw(X, y, Q, isotropic, seed):
    """SpectralMixtureKernel.initialize_from_data in float64 after torch.manual_seed(seed); raw values log(expm1(x))."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).ravel()
    d = X.shape[1]
    maxd = np.empty(d)
    mind = np.empty(d)
    for k in range(d):
        xs = np.sort(X[:, k])
        maxd[k] = xs[-1] - xs[0]
        gaps = np.diff(xs)
        mind[k] = gaps[gaps != 0].min()
    D = d
    if isotropic:
        maxd, mind, D = np.array([maxd.max()]), np.array([mind.min()]), 1
    torch.manual_seed(seed)
    r1 = torch.randn(Q, 1, D, dtype=F64)
    r2 = torch.rand(Q, 1, D, dtype=F64)
    scales = 1.0 / torch.abs(r1 * torch.from_numpy(maxd))
    means = (r2 * 0.5) / torch.from_numpy(mind)
    wv = torch.from_numpy(y).std() / Q
    u = torch.zeros(2 + Q * (2 * D + 1), dtype=F64)
    u[1:1 + Q] = torch.log(torch.expm1(wv))
    u[1 + Q:1 + Q + Q * D] = torch.log(torch.expm1(means)).reshape(-1)
    u[1 + Q + Q * D:1 + Q + 2 * Q * D] = torch.log(torch.expm1(scales)).reshape(-1)
    return u.numpy()


def constrained_row(u, Q, D):
    c, w, m, s, noise = split(torch.as_tensor(u, dtype=F64), Q, D)
    return np.concatenate([[float(c)], w.numpy(), m.reshape(-1).numpy(), s.reshape(-1).numpy(), [float(noise)]])


def fit(u0, X, y, Q, D, lr, T):
    """torch.optim.Adam over u for T steps: (losses before each step, constrained rows after each step, final u)."""
    u = torch.tensor(np.asarray(u0, dtype=np.float64), requires_grad=True)
    opt = torch.optim.Adam([u], lr=lr)
    losses, rows = [], []
    for _ in range(T):
        opt.zero_grad()
        val = loss(u, X, y, Q, D)
        val.backward()
        opt.step()
        losses.append(float(val.item()))
        rows.append(constrained_row(u.detach().numpy(), Q, D))
    return np.array(losses), np.array(rows), u.detach().numpy()


def predict(u, X, y, Xs, Q, D):
    """Predictive mean (c included) and variance of likelihood(model(Xs)) (noise included); NaN rows give NaN."""
    X = torch.as_tensor(X, dtype=F64)
    y = torch.as_tensor(y, dtype=F64)
    Xs = torch.as_tensor(Xs, dtype=F64)
    ut = torch.as_tensor(np.asarray(u, dtype=np.float64))
    c, w, _, _, noise = split(ut, Q, D)
    N = X.shape[0]
    K = kmat(X, X, ut, Q, D) + noise * torch.eye(N, dtype=F64)
    L = torch.linalg.cholesky(K)
    Ks = kmat(X, Xs, ut, Q, D)
    alpha = torch.cholesky_solve((y - c)[:, None], L)[:, 0]
    mean = c + Ks.T @ alpha
    V = torch.linalg.solve_triangular(L, Ks, upper=False)
    var = w.sum() - (V ** 2).sum(0) + noise
    return mean.numpy(), var.numpy()


def random_u(Q, D, seed, scale=0.5):
    """A raw vector with moderate constrained values (means ~ 0.1 .. 0.5 and scales ~ 0.2 .. 0.6 per unit of x)."""
    rng = np.random.default_rng(seed)
    u = np.zeros(2 + Q * (2 * D + 1))
    u[0] = rng.normal() * 0.3
    u[1:1 + Q] = rng.normal(size=Q) * scale - 1.0
    u[1 + Q:1 + Q + Q * D] = np.log(np.expm1(rng.uniform(0.05, 0.4, Q * D)))
    u[1 + Q + Q * D:1 + Q + 2 * Q * D] = np.log(np.expm1(rng.uniform(0.1, 0.4, Q * D)))
    u[-1] = rng.normal() * 0.5 - 2.0
    return u


def random_data(N, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 8.0, size=(N, d))
    y = np.sin(X.sum(1)) + 0.1 * rng.normal(size=N)
    return X, y


def grid_data(N, size, seed):
    """N distinct pixels of a size x size image (integer coordinates, as get_sparse_grid gives them) and smooth values."""
    rng = np.random.default_rng(seed)
    idx = rng.choice(size * size, N, replace=False)
    X = np.stack([idx // size, idx % size], axis=1).astype(np.float64)
    y = np.cos(2 * np.pi * X[:, 0] / 6.0) * np.sin(2 * np.pi * X[:, 1] / 9.0) + 0.05 * rng.normal(size=N)
    return X, y
