"""
CPU references for leave-one-out cross-validation (reconstructor.loo, gpimhip_loo_*), float64 throughout:

  brute(kp, X, y, jitter)    the definition: N refits of the dense oracle, each predicting the point it was not shown
  closed(kp, X, y, jitter)   the identity the engine uses, in numpy: with S = K + (noise + jitter) I, alpha = S^-1 y and
                             d = diag(S^-1):  mean = y - alpha / d,  var = max(1 / d - (noise + jitter), 0) + noise
  score(mean, var, y)        (sum_i log N(y_i | mean_i, var_i), sum_i (y_i - mean_i)^2)
  reflection_assembly(...)   diag(S^-1) and alpha of a complete grid from the reflection blocks of gprutils.reflection_blocks

tests/test_loo_host.py holds closed to brute and the assembly to the dense inverse without a GPU; the GPU tests then trust
closed where brute is too slow.  The problems are those of tests/test_gpu_ops.py (scattered points, `pair` parameters).
"""
import functools
import math

import numpy as np
import torch

from oracle import gpim_oracle as O

JITTER = 1e-5


def scattered(N, d, seed, grid=24):
    """tests/test_gpu_ops.py: N distinct integer points of a grid^d lattice in random order, a noisy sine on them"""
    rng = np.random.default_rng(seed)
    X = np.unique(rng.integers(0, grid, size=(N * 4, d)), axis=0).astype(np.float64)
    rng.shuffle(X)
    X = X[:N]
    y = np.sin(X.sum(1) / 5.0) + 0.1 * rng.standard_normal(len(X))
    return torch.from_numpy(np.ascontiguousarray(X)), torch.from_numpy(y)


def pair(kind, d, ls, seed, jitter=JITTER, noise_u=-3.0):
    """tests/test_gpu_ops.py: (oracle KernelParams, gpim_amd KernelSpec, u) holding identical parameters"""
    from gpim_amd.kernels import KernelSpec
    torch.manual_seed(seed)
    kp = O.KernelParams(kind, d, ls)
    torch.manual_seed(seed)
    spec = KernelSpec(kind, d, ls, jitter=jitter)
    u = spec.draw_initial_u()
    with torch.no_grad():
        kp.u_noise.fill_(noise_u)
    u[1 + spec.n_ls] = noise_u
    return kp, spec, u


def kp_from_u(kind, d, ls, u):
    """The oracle's parameters at the engine's unconstrained vector u = [u_var, u_ls..., u_noise(, u_alpha)]"""
    kp = O.KernelParams(kind, d, ls)
    u = torch.as_tensor(u, dtype=torch.float64).cpu()
    n_ls = kp.u_ls.numel()
    with torch.no_grad():
        kp.u_var.copy_(u[0].reshape(kp.u_var.shape))
        kp.u_ls.copy_(u[1:1 + n_ls].reshape(kp.u_ls.shape))
        kp.u_noise.copy_(u[1 + n_ls])
        if kp.u_alpha is not None:
            kp.u_alpha.copy_(u[2 + n_ls])
    return kp


def problem(kind, N, d, iso, noise_u=-3.0):
    """The (kind, N, d, iso) case of the dense tests: (kp, spec, u, X, y)"""
    X, y = scattered(N, d, seed=N)
    ls = [0.5, 12.0] if iso else [[0.5] * d, [12.0] * d]
    kp, spec, u = pair(kind, d, ls, seed=1, noise_u=noise_u)
    return kp, spec, u, X, y


def brute(kp, X, y, jitter=JITTER):
    """(mean, var) numpy arrays: point i predicted by the dense oracle fitted to the other N - 1 points"""
    N = X.shape[0]
    mean, var = np.empty(N), np.empty(N)
    keep = torch.ones(N, dtype=torch.bool)
    for i in range(N):
        keep[i] = False
        m, v = O.ExactGP(X[keep], y[keep], kp, jitter).predict(X[i:i + 1])
        mean[i], var[i] = m.item(), v.item()
        keep[i] = True
    return mean, var


def closed(kp, X, y, jitter=JITTER):
    """(mean, var) numpy arrays by the closed form, through a Cholesky inverse of S in float64"""
    with torch.no_grad():
        K = kp.K(X).numpy().copy()
        noise = kp.noise.item()
    N = K.shape[0]
    K[np.diag_indices(N)] += jitter + noise
    Li = np.linalg.inv(np.linalg.cholesky(K))
    d = np.einsum("ki,ki->i", Li, Li)
    yn = y.numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
    alpha = Li.T @ (Li @ yn)
    return yn - alpha / d, np.maximum(1.0 / d - (noise + jitter), 0.0) + noise


def score(mean, var, y):
    """(elpd, sse) in float64 from the held-out predictions"""
    mean, var, y = (np.asarray(a, dtype=np.float64) for a in (mean, var, y))
    res = y - mean
    return float(np.sum(-0.5 * (np.log(2.0 * math.pi * var) + res * res / var))), float(np.sum(res * res))


@functools.lru_cache(maxsize=None)
def dense_reference(kind, N, d, iso):
    """The reference of the dense GPU cases, computed once per case: brute up to N = 300, closed beyond"""
    kp, _, _, X, y = problem(kind, N, d, iso)
    return brute(kp, X, y) if N <= 300 else closed(kp, X, y)


def smooth_grid(shape, seed):
    """tests/test_gpu_kron.py: a product of cosines plus noise on a complete grid"""
    rng = np.random.default_rng(seed)
    idx = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    f = np.ones(shape)
    for k, g in enumerate(idx):
        f = f * np.cos(g / (2.0 + k) + 0.3 * k)
    return f + 0.05 * rng.standard_normal(shape)


def reflection_assembly(S, kp, jitter=JITTER):
    """(diag(S^-1), alpha) of the complete grid that S = gprutils.reflection_blocks(X, y, axes) describes, from its blocks:
        K_s[p, q] = w_p w_q sum_g chi_s(g) k(p, g q) + (noise + jitter) [p == q]     (identity rows where w = 0)
        d_i     = sum_{s present at p} (|Stab_p| / B) [K_s^-1]_pp                        p = rep(i)
        alpha_i = sum_s chi_s(sgn_i) sqrt(|Stab_p| / B) (K_s^-1 ys_s)[p]                 |Stab_p| = w_p^-2
    in numpy float64, the arithmetic of loo_finish_kernel's reflection arm."""
    B, dims, Xq = S["B"], S["dims"], S["Xq"]
    Nq = Xq.shape[0]
    wts = S["wts"] if S["wts"] is not None else np.ones((B, Nq))
    with torch.no_grad():
        noise = kp.noise.item()
        Kg = []
        for g in range(B):
            Xg = Xq.copy()
            for j, k in enumerate(dims):
                if (g >> j) & 1:
                    Xg[:, k] = S["twoc"][k] - Xg[:, k]
            Kg.append(kp.K(torch.from_numpy(Xq), torch.from_numpy(Xg)).numpy())
    rep, sgn = S["rep"], S["sgn"]
    d, alpha = np.zeros(len(rep)), np.zeros(len(rep))
    for s in range(B):
        Ks = sum((-1.0 if bin(g & s).count("1") & 1 else 1.0) * Kg[g] for g in range(B))
        w = wts[s]
        Ks = Ks * np.outer(w, w) + (noise + jitter) * np.eye(Nq)
        gone = w == 0.0
        Ks[gone, :] = 0.0
        Ks[:, gone] = 0.0
        Ks[gone, gone] = 1.0
        Ki = np.linalg.inv(Ks)
        a_s = Ki @ S["ys"][s]
        present = ~gone[rep]
        c = np.zeros(len(rep))
        c[present] = 1.0 / (w[rep][present] * math.sqrt(B))
        chi = np.where(np.array([bin(int(g) & s).count("1") & 1 for g in sgn]) == 1, -1.0, 1.0)
        d += c * c * np.diag(Ki)[rep]
        alpha += chi * c * a_s[rep]
    return d, alpha
