"""
CPU references for the leave-one-out objective (reconstructor(objective='loo'), gpimhip_loo_grad, gpimhip_fit_exact_loo;
DESIGN.md section 31), float64 throughout.  With S = K + (noise + jitter) I, alpha = S^-1 y and d = diag(S^-1)

    loss(u) = sum_i [ -1/2 log d_i + alpha_i^2 / (2 d_i) ] + N/2 log 2 pi + prior constant

  autograd(kp, X, y, jitter)   (loss, gradient): torch autograd through an explicit inverse of S
  closed(kp, X, y, jitter)     (loss, gradient): numpy, through a Cholesky inverse, with q = alpha / d, r = S^-1 q,
                               omega = 1 / d + q^2, G2 = S^-1 diag(omega) S^-1 and
                               d loss / d theta = 1/2 sum_ij dS_ij/d theta (G2_ij - (r_i alpha_j + alpha_i r_j)):
                               the arithmetic of the engine, with the kernel's derivatives written out by hand
  adam_path(kp, X, y, ...)     torch.optim.Adam on autograd's loss: (history rows, losses)

Both gradients are in the engine's order u_var, u_ls..., u_noise(, u_alpha).  The two share the kernel matrix's definition
(oracle.gpim_oracle.KernelParams) and nothing else.  The problems are those of tests/loo_oracle.py.
"""
import functools
import math

import numpy as np
import torch

import loo_oracle as LO

JITTER = LO.JITTER

# (kernel, N, d, isotropic): the smallest shapes where each index path of the engine can break (tests/test_gpu_loo_objective.py)
CASES = [("RBF", 7, 2, False), ("Matern52", 40, 2, False), ("RBF", 130, 3, False), ("Matern52", 257, 4, False),
         ("RationalQuadratic", 200, 3, False), ("RBF", 300, 2, True), ("Matern52", 530, 3, False)]


def loss_torch(kp, X, y, jitter=JITTER):
    """The objective as a differentiable torch scalar, through torch.linalg.inv"""
    N = X.shape[0]
    S = kp.K(X) + (kp.noise + jitter) * torch.eye(N, dtype=torch.float64)
    Si = torch.linalg.inv(S)
    alpha, d = Si @ y, Si.diagonal()
    return (-0.5 * d.log() + 0.5 * alpha * alpha / d).sum() + 0.5 * N * math.log(2.0 * math.pi) + kp.neg_log_prior()


def autograd(kp, X, y, jitter=JITTER):
    """(loss, gradient) numpy float64 by torch autograd"""
    ps = kp.parameters()
    for p in ps:
        p.grad = None
    loss = loss_torch(kp, X, y, jitter)
    loss.backward()
    return loss.item(), torch.cat([p.grad.reshape(-1) for p in ps]).numpy().copy()


def _interval(u, lo, hi):
    """value and d value / du of the clipped-sigmoid interval map (0 where it saturates)"""
    fi = np.finfo(np.float64)
    s = 1.0 / (1.0 + np.exp(-u))
    ds = s * (1.0 - s)
    sat = (s < fi.tiny) | (s > 1.0 - fi.eps)
    s = np.clip(s, fi.tiny, 1.0 - fi.eps)
    return lo + (hi - lo) * s, np.where(sat, 0.0, (hi - lo) * ds)


def closed(kp, X, y, jitter=JITTER):
    """(loss, gradient) numpy float64 by the G2 / r formula"""
    Xn = X.numpy() if isinstance(X, torch.Tensor) else np.asarray(X, dtype=np.float64)
    yn = y.numpy() if isinstance(y, torch.Tensor) else np.asarray(y, dtype=np.float64)
    N, dim = Xn.shape
    with torch.no_grad():
        u_var, u_ls, u_noise = kp.u_var.numpy().copy(), kp.u_ls.numpy().reshape(-1).copy(), float(kp.u_noise)
        u_a = None if kp.u_alpha is None else float(kp.u_alpha)
        lo_v, hi_v = float(kp.amp_lo), float(kp.amp_hi)
        lo_l, hi_l = kp.ls_lo.numpy().reshape(-1), kp.ls_hi.numpy().reshape(-1)
        prior = float(kp.neg_log_prior())
    var, dvar = _interval(u_var, lo_v, hi_v)
    var, dvar = float(var), float(dvar)
    ls, dls = _interval(u_ls, lo_l, hi_l)
    n_ls = ls.size
    lsd = np.broadcast_to(ls, (dim,)) if n_ls == 1 else ls
    noise = math.exp(u_noise)
    diff2 = ((Xn[:, None, :] - Xn[None, :, :]) / lsd) ** 2                 # (N, N, dim): scaled squared differences
    r2 = diff2.sum(-1)
    # k = var * e(r2);  dk / d r2 = var * h(r2)
    if kp.kind == "RBF":
        e = np.exp(-0.5 * r2)
        h = -0.5 * e
        ga = None
    elif kp.kind == "Matern52":
        r = np.sqrt(r2 + 1e-12)
        s5r = math.sqrt(5.0) * r
        ex = np.exp(-s5r)
        e = (1.0 + s5r + (5.0 / 3.0) * r2) * ex
        # d/dr2: dr/dr2 = 1 / (2 r) on the shifted r, the (5/3) r2 term un-shifted (the oracle's definition)
        h = ((math.sqrt(5.0) / (2.0 * r)) + 5.0 / 3.0) * ex - (1.0 + s5r + (5.0 / 3.0) * r2) * ex * math.sqrt(5.0) / (2.0 * r)
        ga = None
    else:
        a = math.exp(u_a)
        base = 1.0 + (0.5 / a) * r2
        e = base ** (-a)
        h = -0.5 * base ** (-a - 1.0)
        ga = e * (-np.log(base) + (0.5 * r2 / a) / base)                   # d e / d a
    S = var * e
    S[np.diag_indices(N)] += noise + jitter
    Li = np.linalg.inv(np.linalg.cholesky(S))
    Si = Li.T @ Li
    alpha = Li.T @ (Li @ yn)
    d = np.einsum("ki,ki->i", Li, Li)
    q = alpha / d
    rv = Li.T @ (Li @ q)
    omega = 1.0 / d + q * q
    G2 = (Si * omega) @ Si
    M = G2 - (np.outer(rv, alpha) + np.outer(alpha, rv))
    loss = float(np.sum(-0.5 * np.log(d) + 0.5 * alpha * q)) + 0.5 * N * math.log(2.0 * math.pi) + prior
    g = [0.5 * np.sum(M * e) * dvar]
    # d r2 / d l_k = -2 diff2_k / l_k
    gl = np.array([0.5 * np.sum(M * var * h * (-2.0) * diff2[:, :, k]) / lsd[k] for k in range(dim)])
    g += [gl.sum() * dls[0]] if n_ls == 1 else list(gl * dls)
    g.append(0.5 * np.trace(M) * noise)
    if ga is not None:
        g.append(0.5 * np.sum(M * var * ga) * a)
    return loss, np.array(g, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def reference(kind, N, d, iso):
    """autograd's (loss, gradient) of the (kind, N, d, iso) case of loo_oracle.problem, computed once per case"""
    kp, _, _, X, y = LO.problem(kind, N, d, iso)
    return autograd(kp, X, y)


def spread(a, b):
    """(relative loss difference, largest absolute gradient difference) of two (loss, gradient) pairs"""
    return abs(a[0] - b[0]) / abs(b[0]), float(np.abs(a[1] - b[1]).max())


def adam_path(kp, X, y, lr, steps, jitter=JITTER, loss_fn=None):
    """torch.optim.Adam on the objective (tests/test_gpu_ops.py: test_fit_trajectory's loop): the constrained values after
    every step, rows [variance, lengthscales..., noise(, alpha)], and the loss before every step"""
    loss_fn = loss_fn or loss_torch
    ps = kp.parameters()
    opt = torch.optim.Adam(ps, lr=lr)
    hist, losses = [], []
    for _ in range(steps):
        opt.zero_grad()
        loss = loss_fn(kp, X, y, jitter)
        loss.backward()
        opt.step()
        with torch.no_grad():
            row = [kp.variance.reshape(-1), kp.lengthscale.reshape(-1), kp.noise.reshape(-1)]
            if kp.u_alpha is not None:
                row.append(kp.scale_mixture.reshape(-1))
            hist.append(torch.cat(row).numpy().copy())
        losses.append(loss.item())
    return np.array(hist), np.array(losses)
