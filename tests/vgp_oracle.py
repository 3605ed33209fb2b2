"""Test-side oracles of the exact multi-output GP (gpim_amd.vreconstructor, reference gpim/gpreg/vgpr.py).

* ``Dense``: the model restated without the block reduction -- the N T x N T covariance C = B (x) K + diag(s) (x) I built
  explicitly, torch.linalg.cholesky, autograd, torch.optim.Adam over the raw vector, the analytic predictive (CPU,
  float64).  It checks the engine's reduction independently.
* ``reduction_loss_grad``: the reduction's own loss and gradient formulas in numpy -- T dense
  N x N blocks lambda_t K + I -- for the CPU tests and the full-size twin where the dense N T system is too large.

Raw vector (include/gpimhip.h): u = [mu (T) | F (T) or r_o (T) | r_v (T, correlated only) | r_l (n_ls) | r_a (T) | r_g].
The covariance functions follow the engine's (csrc/kfun.hpp): RBF exp(-r2/2), Matern52 with r = sqrt(r2 + 1e-12).
"""
import math

import numpy as np
import torch

F64 = torch.float64
SQRT5 = 5.0 ** 0.5


def layout(T, n_ls, independent):
    o = {"mu": slice(0, T)}
    if independent:
        o["scale"] = slice(T, 2 * T)
        p = 2 * T
    else:
        o["F"] = slice(T, 2 * T)
        o["rv"] = slice(2 * T, 3 * T)
        p = 3 * T
    o["ls"] = slice(p, p + n_ls)
    o["noise"] = slice(p + n_ls, p + n_ls + T)
    o["global"] = p + n_ls + T
    return o, p + n_ls + T + 1


def params_torch(u, T, n_ls, independent, bounds):
    """(mu, B, s, l) as differentiable torch functions of u."""
    sp = torch.nn.functional.softplus
    o, _ = layout(T, n_ls, independent)
    mu = u[o["mu"]]
    if independent:
        B = torch.diag(sp(u[o["scale"]]))
    else:
        F = u[o["F"]].reshape(T, 1)
        B = F @ F.T + torch.diag(sp(u[o["rv"]]))
    r = u[o["ls"]]
    if bounds is None:
        ls = sp(r)
    else:
        lo = torch.as_tensor(np.broadcast_to(bounds[0], (n_ls,)).copy(), dtype=F64)
        hi = torch.as_tensor(np.broadcast_to(bounds[1], (n_ls,)).copy(), dtype=F64)
        ls = torch.sigmoid(r) * (hi - lo) + lo
    s = (1e-4 + sp(u[o["noise"]])) + (1e-4 + sp(u[o["global"]]))
    return mu, B, s, ls


def kmat_torch(Xa, Xb, ls, kernel):
    d = Xa.shape[1]
    l = ls.expand(d) if ls.numel() == 1 else ls
    a, b = Xa / l, Xb / l
    r2 = torch.clamp((a * a).sum(1)[:, None] - 2.0 * a @ b.T + (b * b).sum(1)[None, :], min=0.0)
    if kernel == "RBF":
        return torch.exp(-0.5 * r2)
    r = torch.sqrt(r2 + 1e-12)
    return (1.0 + SQRT5 * r + (5.0 / 3.0) * r2) * torch.exp(-SQRT5 * r)


class Dense:
    """The dense restatement for one data set: X (N x d), Y (N x T) numpy arrays."""

    def __init__(self, X, Y, kernel="RBF", independent=False, bounds=None, isotropic=False):
        self.X = torch.as_tensor(np.asarray(X, dtype=np.float64))
        self.Y = torch.as_tensor(np.asarray(Y, dtype=np.float64))
        self.N, self.T = self.Y.shape
        self.kernel, self.independent, self.bounds = kernel, independent, bounds
        self.n_ls = 1 if isotropic else self.X.shape[1]
        self.P = layout(self.T, self.n_ls, independent)[1]

    def params(self, u):
        return params_torch(torch.as_tensor(u, dtype=F64), self.T, self.n_ls, self.independent, self.bounds)

    def loss(self, u):
        mu, B, s, ls = params_torch(u, self.T, self.n_ls, self.independent, self.bounds)
        N, T = self.N, self.T
        K = kmat_torch(self.X, self.X, ls, self.kernel)
        C = torch.kron(B, K) + torch.kron(torch.diag(s), torch.eye(N, dtype=F64))
        r = (self.Y - mu[None, :]).T.reshape(-1)
        L = torch.linalg.cholesky(C)
        a = torch.cholesky_solve(r[:, None], L)[:, 0]
        nll = 0.5 * (r @ a) + torch.log(torch.diagonal(L)).sum() + 0.5 * N * T * math.log(2 * math.pi)
        return nll / (N * T)

    def loss_grad(self, u):
        u = torch.tensor(np.asarray(u, dtype=np.float64), requires_grad=True)
        loss = self.loss(u)
        loss.backward()
        return float(loss.item()), u.grad.numpy().copy()

    def fit(self, u0, lr, iters):
        """torch.optim.Adam over the raw vector (vgpr.py:141-176): lengthscales after every step, losses before, final u."""
        u = torch.tensor(np.asarray(u0, dtype=np.float64), requires_grad=True)
        opt = torch.optim.Adam([u], lr=lr)
        hist, losses = [], []
        for _ in range(iters):
            opt.zero_grad()
            loss = self.loss(u)
            loss.backward()
            opt.step()
            losses.append(float(loss.item()))
            with torch.no_grad():
                hist.append(self.params(u.detach())[3].numpy().copy())
        return np.array(hist), np.array(losses), u.detach().numpy().copy()

    def predict(self, u, Xs):
        """Exact predictive mean / variance of likelihood(model(Xs)), M x T each (NaN rows give NaN)."""
        with torch.no_grad():
            mu, B, s, ls = self.params(u)
            N, T = self.N, self.T
            Xs = torch.as_tensor(np.asarray(Xs, dtype=np.float64))
            K = kmat_torch(self.X, self.X, ls, self.kernel)
            Ks = kmat_torch(self.X, Xs, ls, self.kernel)                 # N x M
            C = torch.kron(B, K) + torch.kron(torch.diag(s), torch.eye(N, dtype=F64))
            L = torch.linalg.cholesky(C)
            r = (self.Y - mu[None, :]).T.reshape(-1)
            alpha = torch.cholesky_solve(r[:, None], L)[:, 0].reshape(T, N)
            mean = mu[None, :] + (Ks.T @ alpha.T) @ B                    # mean_a = mu_a + sum_b B_ab k*^T alpha_b
            var = torch.empty_like(mean)
            for a in range(T):
                W = torch.linalg.solve_triangular(L, torch.kron(B[:, a:a + 1], Ks), upper=False)
                var[:, a] = B[a, a] + s[a] - (W * W).sum(0)
            return mean.numpy(), var.numpy()


# ---------------------------------------------------------------------------------------------------------------------
# the reduction, restated in numpy
# ---------------------------------------------------------------------------------------------------------------------
def _softplus(x):
    return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _kmat_np(X, ls, kernel):
    """K and dK/dl_k (k over the n_ls lengthscales)."""
    d = X.shape[1]
    l = np.broadcast_to(ls, (d,)) if ls.size == 1 else ls
    a = X / l
    sq = (a * a).sum(1)
    r2 = np.maximum(sq[:, None] - 2.0 * a @ a.T + sq[None, :], 0.0)
    if kernel == "RBF":
        K = np.exp(-0.5 * r2)
        h = K
    else:
        r = np.sqrt(r2 + 1e-12)
        ex = np.exp(-SQRT5 * r)
        K = (1.0 + SQRT5 * r + (5.0 / 3.0) * r2) * ex
        h = (5.0 / 3.0) * (1.0 + SQRT5 * (r2 / r)) * ex
    dK = [h * (a[:, k][:, None] - a[:, k][None, :]) ** 2 / l[k] for k in range(d)]
    if ls.size == 1:
        dK = [sum(dK)]
    return K, dK


def reduction_loss_grad(u, X, Y, kernel="RBF", independent=False, bounds=None, isotropic=False):
    """Loss and gradient through the exact block reduction (eigen-decomposition of B~, T blocks lambda_t K + I)."""
    u = np.asarray(u, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    N, T = Y.shape
    n_ls = 1 if isotropic else X.shape[1]
    o, P_len = layout(T, n_ls, independent)
    mu = u[o["mu"]]
    if independent:
        rd = u[o["scale"]]
        B = np.diag(_softplus(rd))
    else:
        F = u[o["F"]].reshape(T, 1)
        rd = u[o["rv"]]
        B = F @ F.T + np.diag(_softplus(rd))
    r = u[o["ls"]]
    if bounds is None:
        ls, dls = _softplus(r), _sigmoid(r)
    else:
        lo, hi = (np.broadcast_to(np.asarray(b, dtype=np.float64), (n_ls,)) for b in bounds)
        sg = _sigmoid(r)
        ls, dls = sg * (hi - lo) + lo, (hi - lo) * sg * (1 - sg)
    ra, rg = u[o["noise"]], u[o["global"]]
    s = (1e-4 + _softplus(ra)) + (1e-4 + _softplus(rg))
    Bt = B / np.sqrt(np.outer(s, s))
    lam, Q = np.linalg.eigh(Bt)
    Pm = Q / np.sqrt(s)[:, None]
    Z = (Y - mu[None, :]) @ Pm                      # z_t = sum_a P_at (y_a - mu_a)
    K, dK = _kmat_np(X, ls, kernel)
    Bm = np.empty((N, T))
    lg = q = 0.0
    trMK, trM = np.empty(T), np.empty(T)
    gl = np.zeros(n_ls)
    for t in range(T):
        A = lam[t] * K + np.eye(N)
        L = np.linalg.cholesky(A)
        M = np.linalg.inv(A)
        b = M @ Z[:, t]
        Bm[:, t] = b
        lg += np.log(np.diag(L)).sum()
        q += Z[:, t] @ b
        trMK[t] = (M * K).sum()
        trM[t] = np.trace(M)
        for k in range(n_ls):
            gl[k] += 0.5 * lam[t] * ((M * dK[k]).sum() - b @ dK[k] @ b)
    G, H, sig = Bm.T @ K @ Bm, Bm.T @ Bm, Bm.sum(0)
    gB = 0.5 * (Pm @ np.diag(trMK) @ Pm.T - Pm @ G @ Pm.T)
    gs = 0.5 * (np.diag(Pm @ np.diag(trM) @ Pm.T) - np.diag(Pm @ H @ Pm.T))
    g = np.zeros(P_len)
    g[o["mu"]] = -Pm @ sig
    if independent:
        g[o["scale"]] = np.diag(gB) * _sigmoid(rd)
    else:
        g[o["F"]] = ((gB + gB.T) @ F).reshape(-1)
        g[o["rv"]] = np.diag(gB) * _sigmoid(rd)
    g[o["ls"]] = gl * dls
    g[o["noise"]] = gs * _sigmoid(ra)
    g[o["global"]] = gs.sum() * _sigmoid(rg)
    nt = N * T
    loss = (0.5 * N * np.log(s).sum() + lg + 0.5 * q) / nt + 0.5 * math.log(2 * math.pi)
    return loss, g / nt


def initial_u(T, n_ls, independent, seed=0):
    """The reference's initial raw vector: F = torch.randn(T, 1) right after manual_seed(seed), everything else 0."""
    _, P = layout(T, n_ls, independent)
    u = np.zeros(P)
    if not independent:
        torch.manual_seed(seed)
        u[T:2 * T] = torch.randn(T, 1, dtype=F64).numpy().reshape(-1)
    return u


def random_data(N, T, d, seed, scale=1.0):
    """N scattered points in [0, 8]^d and T correlated smooth outputs."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 8.0, size=(N, d))
    base = np.stack([np.sin(X @ rng.normal(size=d) * 0.6 + rng.uniform(0, 6)) for _ in range(3)], 1)
    W = rng.normal(size=(3, T))
    Y = scale * (base @ W + 0.1 * rng.normal(size=(N, T)) + rng.normal(size=T))
    return X, Y


def random_u(T, n_ls, independent, seed):
    rng = np.random.default_rng(seed)
    _, P = layout(T, n_ls, independent)
    return rng.normal(scale=0.7, size=P)
