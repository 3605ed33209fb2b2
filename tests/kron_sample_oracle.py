"""
Dense numpy oracle of the Kronecker posterior draws (reconstructor.sample(method='kron')).

  * ``posterior``   the exact GP posterior on a product test grid from the full kernel matrices and a Cholesky factor:
                    nothing Kronecker in it.
  * ``draw_matrix`` the rule of the feature restated with numpy.linalg.eigh: the matrix A of ``out = mean + A z`` for
                    z = [zeta | z_e | z_n].  The root of the prior is fixed only up to an orthogonal change of zeta, so A is
                    comparable between implementations through A A^T alone -- which must be Sigma_post + c I.
  * ``CASES``       the grids and hyper-parameters shared by the host test and the GPU test.

RBF kernel of the engine: k(x, x') = s2 prod_i exp(-((x_i - x'_i) / l_i)^2 / 2); sigma = noise + the model's jitter on the
training diagonal; c = (0 if noiseless else noise) + jitter on the draws.
"""
import functools

import numpy as np

from gpim_amd.gprutils import union_axes

MODEL_JITTER = 1e-5


def axis_kernel(a, b, l):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.exp(-0.5 * ((a[:, None] - b[None, :]) / l) ** 2)


def points(axes):
    return np.stack(np.meshgrid(*[np.asarray(a, dtype=np.float64) for a in axes], indexing="ij"), -1).reshape(-1, len(axes))


def full_kernel(A, B, ls, s2):
    """K(A, B) of the rows A (n, d), B (m, d): built point by point, no Kronecker product"""
    ls = np.asarray(ls, dtype=np.float64)
    D = (A[:, None, :] - B[None, :, :]) / ls
    return s2 * np.exp(-0.5 * (D ** 2).sum(-1))


def posterior(c, t, ls, s2, noise, model_jitter, y=None):
    """(mean, Sigma_post) on the product grid of the axes t for observations y (grid order) on the product grid of the axes
    c; mean is None without y.  Sigma_post has no noise and no jitter on its diagonal."""
    X, Xs = points(c), points(t)
    K = full_kernel(X, X, ls, s2) + (noise + model_jitter) * np.eye(len(X))
    Ks = full_kernel(Xs, X, ls, s2)
    L = np.linalg.cholesky(K)
    V = np.linalg.solve(L, Ks.T)
    cov = full_kernel(Xs, Xs, ls, s2) - V.T @ V
    mean = None if y is None else V.T @ np.linalg.solve(L, np.asarray(y, dtype=np.float64).ravel())
    return mean, cov


def kron_all(mats):
    return functools.reduce(np.kron, mats)


def draw_matrix(c, t, ls, s2, noise, model_jitter, noiseless, jitter):
    """A (M, prod U_i + N + M) with out = mean + A [zeta | z_e | z_n]:
        A = [ sqrt(s2) (Rt - s2 Ks_ Q D^-1 Q^T Rg) | -s2 sqrt(sigma) Ks_ Q D^-1 Q^T | sqrt(c) I ]
    Rg = (x) R_i[ic_i, :], Rt = (x) R_i[it_i, :], R_i = Q_i^U sqrt(max(lam_i^U, 0)) from eigh of K_i on the union axis;
    Ks_ = (x) K_i(t_i, c_i), Q = (x) Q_i, D = s2 (x) lam_i + sigma from eigh of K_i on the training axis."""
    sigma = noise + model_jitter
    cc = (0.0 if noiseless else noise) + jitter
    au, ic, it = union_axes(c, t)
    Rg, Rt, Qs, lams, Kss = [], [], [], [], []
    for i, l in enumerate(ls):
        lam_u, Q_u = np.linalg.eigh(axis_kernel(au[i], au[i], l))
        R = Q_u * np.sqrt(np.maximum(lam_u, 0.0))
        Rg.append(R[ic[i]])
        Rt.append(R[it[i]])
        lam, Q = np.linalg.eigh(axis_kernel(c[i], c[i], l))
        Qs.append(Q)
        lams.append(lam)
        Kss.append(axis_kernel(t[i], c[i], l))
    Rg, Rt, Q, Ks = kron_all(Rg), kron_all(Rt), kron_all(Qs), kron_all(Kss)
    D = s2 * kron_all(lams) + sigma
    G = s2 * ((Ks @ Q) / D) @ Q.T                  # K(test, train) (K + sigma I)^-1: the update's matrix, M x N
    M = Ks.shape[0]
    return np.hstack([np.sqrt(s2) * (Rt - G @ Rg), -np.sqrt(sigma) * G, np.sqrt(cc) * np.eye(M)])


def widths(c, t):
    """(prod U_i, N, M) of a case"""
    au = union_axes(c, t)[0]
    return (int(np.prod([len(a) for a in au])), int(np.prod([len(a) for a in c])), int(np.prod([len(a) for a in t])))


def _r(n):
    return np.arange(n, dtype=np.float64)


GRID_65 = (_r(6), _r(5))
PARAMS_2D = (([1.5, 2.5], 0.8, 0.05), ([6.0, 9.0], 3.0, 1e-3), ([0.4, 0.6], 9.0, 1e-4))
PARAMS_3D = (([1.2, 2.0, 1.7], 1.3, 0.02),)
PARAMS_4D = (([1.2, 2.0, 1.7, 0.9], 1.3, 0.02),)
# name -> (training axes, test axes, parameter sets)
GRIDS = {
    "same": (GRID_65, GRID_65, PARAMS_2D),
    "finer": (GRID_65, (np.arange(0, 5.5, .5), np.arange(0, 4.5, .5)), PARAMS_2D),
    "shifted": (GRID_65, (_r(6) + 0.37, np.linspace(-1, 5, 7)), PARAMS_2D),
    "crop": (GRID_65, (np.array([1., 2., 3.]), np.array([2., 3., 4.])), PARAMS_2D),
    "3d": ((_r(4), _r(3), _r(5)), (np.arange(0, 3.5, .5), _r(3), np.array([0.25, 3.3])), PARAMS_3D),
    "4d": ((_r(3), _r(2), _r(3), _r(2)), (np.arange(0, 2.5, .5), _r(2), np.array([0.5, 1.5]), _r(2)), PARAMS_4D),
}
CASES = tuple((name, k) for name, g in GRIDS.items() for k in range(len(g[2])))


def case(name, k):
    """(c, t, ls, s2, noise) of CASES entry (name, k)"""
    c, t, params = GRIDS[name]
    ls, s2, noise = params[k]
    return c, t, ls, s2, noise
