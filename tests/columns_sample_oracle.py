"""A dense numpy restatement of the posterior draws of the dense-by-Kronecker blocks (DESIGN.md section 23,
gpimhip_sample_pkron): Matheron's rule with the prior drawn through chol(s2 K_s(P, P) + d I) of the union P of the ragged
rows and the eigen-roots of the union of the complete axes, every matrix formed in full (np.linalg.cholesky, eigh, kron).

Everything here is in the library's layouts: training points as (N_s, J), test points as (M_s, M_c), ragged axes first.
``rule`` returns the matrix A of ``out = mean + A z`` (z = [zeta | z_e | z_n]), the dense posterior covariance and the
closed-form extra term d T (I (x) K_c(u, u)) T^T, so that A A^T = Sigma_post + c_n I + extra."""
from functools import reduce

import numpy as np

from columns_oracle import rbf
from gpim_amd import gprutils

MODEL_JITTER = 1e-5          # kernels.get_kernel's default, the model's diag_add beside the noise
D = 1e-5                     # the jitter argument of the draws

# (s2, ragged lengthscales, lengthscale of every complete axis, noise)
PARAMS = ((1.3, (2.0, 2.5), 1.5, 0.05), (0.7, (4.0, 3.0), 60.0, 1e-3))


def kron_all(mats):
    return reduce(np.kron, mats)


def rbf1(a, b, l):
    return np.exp(-0.5 * ((np.asarray(a)[:, None] - np.asarray(b)[None, :]) / l) ** 2)


def widths(Xs, axes_c, Xt, axes_t):
    """(U_s, U, N, M) of a draw from the training rows / axes on the test rows / axes."""
    P = gprutils.union_rows(Xs, Xt)[0]
    au = gprutils.union_axes(axes_c, axes_t)[0]
    U = int(np.prod([len(a) for a in au]))
    return len(P), U, len(Xs) * int(np.prod([len(c) for c in axes_c])), len(Xt) * int(np.prod([len(t) for t in axes_t]))


def rule(Xs, axes_c, Y, Xt, axes_t, var, ls_r, ls_c, noise, jitter, d, noiseless):
    """(A (M x W), mean (M), Sigma_post (M x M), extra (M x M)); W = U_s U + N + M."""
    Xs, Xt = np.asarray(Xs, dtype=np.float64), np.asarray(Xt, dtype=np.float64)
    P, iX, iT = gprutils.union_rows(Xs, Xt)
    au, ic, it = gprutils.union_axes(axes_c, axes_t)
    sigma = noise + jitter
    LP = np.linalg.cholesky(var * rbf(P, P, np.asarray(ls_r)) + d * np.eye(len(P)))
    R, Ku = [], []
    for a, l in zip(au, ls_c):
        K = rbf1(a, a, l)
        lam, Q = np.linalg.eigh(K)
        R.append(Q * np.sqrt(np.maximum(lam, 0.0)))
        Ku.append(K)
    RX = kron_all([r[i] for r, i in zip(R, ic)])                  # J x U
    RT = kron_all([r[i] for r, i in zip(R, it)])                  # M_c x U
    GX, GT = np.kron(LP[iX], RX), np.kron(LP[iT], RT)             # the prior on the training / test points from zeta
    Kc = kron_all([rbf1(c, c, l) for c, l in zip(axes_c, ls_c)])
    Ktc = kron_all([rbf1(t, c, l) for t, c, l in zip(axes_t, axes_c, ls_c)])
    Ktt = kron_all([rbf1(t, t, l) for t, l in zip(axes_t, ls_c)])
    KXX = var * np.kron(rbf(Xs, Xs, np.asarray(ls_r)), Kc)
    KtX = var * np.kron(rbf(Xt, Xs, np.asarray(ls_r)), Ktc)
    N, M = KXX.shape[0], KtX.shape[0]
    Wm = np.linalg.solve(KXX + sigma * np.eye(N), KtX.T).T       # K_*X (K_XX + sigma I)^-1
    cn = 0.0 if noiseless else noise
    A = np.concatenate([GT - Wm @ GX, -np.sqrt(sigma) * Wm, np.sqrt(cn) * np.eye(M)], axis=1)
    mean = Wm @ np.asarray(Y, dtype=np.float64).reshape(-1)
    cov = var * np.kron(rbf(Xt, Xt, np.asarray(ls_r)), Ktt) - Wm @ KtX.T
    # T = S_* - W S_X with S the selections out of the union product grid P x u
    Iu = [np.eye(len(a)) for a in au]
    SX = np.kron(np.eye(len(P))[iX], kron_all([e[i] for e, i in zip(Iu, ic)]))
    ST = np.kron(np.eye(len(P))[iT], kron_all([e[i] for e, i in zip(Iu, it)]))
    T = ST - Wm @ SX
    extra = d * T @ np.kron(np.eye(len(P)), kron_all(Ku)) @ T.T
    return A, mean, cov, extra
