"""A numpy restatement of the dense-by-Kronecker blocks (csrc/pkron.hip): loss, gradient, posterior
mean and variance of the exact RBF GP on (observed ragged points) x (complete axes), block by block.  float64 throughout;
the arithmetic follows the engine's formulas, not its launch structure."""
import numpy as np

LOG2PI = 1.8378770664093453


def rbf(a, b, ls):
    d = a[:, None, :] / ls - b[None, :, :] / ls
    return np.exp(-0.5 * (d * d).sum(-1))


def _axes(axes_c, ls_c):
    """Per complete axis: lambda (clamped at 0), Q, Mm = Q^T E Q with E = K o ((c_a - c_b) / l)^2 = l dK / dl."""
    out = []
    for c, l in zip(axes_c, ls_c):
        r2 = ((c[:, None] - c[None, :]) / l) ** 2
        K = np.exp(-0.5 * r2)
        lam, Q = np.linalg.eigh(K)
        out.append((np.maximum(lam, 0.0), Q, Q.T @ (K * r2) @ Q))
    return out


def _mode(T, M, axis):
    """T x_axis M: out[..., a, ...] = sum_b M[a, b] T[..., b, ...]."""
    return np.moveaxis(np.tensordot(M, T, axes=(1, axis)), 0, axis)


def _blocks(Xs, axes_c, Y, var, ls_r, ls_c, noise, jitter):
    ax = _axes(axes_c, ls_c)
    nc = [len(c) for c in axes_c]
    lam = np.ones(())
    for l, _, _ in ax:
        lam = np.multiply.outer(lam, l)
    lam = lam.ravel()
    Yt = Y.reshape([Y.shape[0]] + nc)
    for i, (_, Q, _) in enumerate(ax):
        Yt = _mode(Yt, Q.T, 1 + i)
    Yt = Yt.reshape(Y.shape[0], -1)
    Ks = rbf(Xs, Xs, ls_r)
    sigma = noise + jitter
    Minv, beta, logdet = [], [], 0.0
    for j in range(len(lam)):
        A = var * lam[j] * Ks + sigma * np.eye(len(Xs))
        L = np.linalg.cholesky(A)
        Mi = np.linalg.inv(A)
        Minv.append(Mi)
        beta.append(Mi @ Yt[:, j])
        logdet += 2.0 * np.log(np.diag(L)).sum()
    return ax, nc, lam, Yt, Ks, np.array(Minv), np.array(beta).T, logdet


def loss_grad(Xs, axes_c, Y, var, ls_r, ls_c, noise, jitter):
    """(loss without the priors' constant, d/d var, d/d ls_r (p), d/d ls_c (dc), d/d noise) at the constrained values."""
    ax, nc, lam, Yt, Ks, Minv, B, logdet = _blocks(Xs, axes_c, Y, var, ls_r, ls_c, noise, jitter)
    Ns, J = Yt.shape
    loss = 0.5 * ((Yt * B).sum() + logdet) + 0.5 * Ns * J * LOG2PI
    r2 = [((Xs[:, None, k] - Xs[None, :, k]) / ls_r[k]) ** 2 for k in range(Xs.shape[1])]
    S0, Sk, S5 = np.zeros(J), np.zeros((len(r2), J)), np.zeros(J)
    for j in range(J):
        G = Minv[j] - np.outer(B[:, j], B[:, j])
        S0[j] = (G * Ks).sum()
        for k in range(len(r2)):
            Sk[k, j] = (G * Ks * r2[k]).sum()
        S5[j] = np.trace(G)
    dvar = 0.5 * (lam * S0).sum()
    dls_r = np.array([0.5 * var * (lam * Sk[k]).sum() / ls_r[k] for k in range(len(r2))])
    dnoise = 0.5 * S5.sum()
    W = Ks @ B
    trmk = (S0 + (B * W).sum(0)).reshape(nc)                      # tr(M_j K_s)
    dls_c = np.zeros(len(ax))
    for i in range(len(ax)):
        WF = W.reshape([Ns] + nc)
        po = np.ones(())
        for k, (l, _, Mm) in enumerate(ax):
            if k == i:
                WF = _mode(WF, Mm, 1 + k)
                po = np.multiply.outer(po, np.diag(Mm))
            else:
                shape = [1] * (1 + len(nc))
                shape[1 + k] = -1
                WF = WF * l.reshape(shape)
                po = np.multiply.outer(po, l)
        dls_c[i] = 0.5 * var * ((po * trmk).sum() - (B * WF.reshape(Ns, J)).sum()) / ls_c[i]
    return loss, dvar, dls_r, dls_c, dnoise


def predict(Xs, axes_c, Y, var, ls_r, ls_c, noise, jitter, Xs_test, axes_test_c):
    """Posterior mean and variance (noise included) on (ragged test rows) x (product of the complete test axes): M_s x M_c."""
    ax, nc, lam, Yt, Ks, Minv, B, _ = _blocks(Xs, axes_c, Y, var, ls_r, ls_c, noise, jitter)
    Kst = rbf(Xs_test, Xs, ls_r)                                   # M_s x N_s, variance 1
    G = Kst @ B                                                   # M_s x J
    q = np.stack([((Kst @ Minv[j]) * Kst).sum(1) for j in range(len(lam))], axis=1)
    Ms = len(Xs_test)
    Gm, Qv = G.reshape([Ms] + nc), q.reshape([Ms] + nc)
    for i, ((_, Q, _), c, ct, l) in enumerate(zip(ax, axes_c, axes_test_c, ls_c)):
        b = np.exp(-0.5 * ((ct[:, None] - c[None, :]) / l) ** 2) @ Q
        Gm, Qv = _mode(Gm, b, 1 + i), _mode(Qv, b * b, 1 + i)
    mean = var * Gm.reshape(Ms, -1)
    v = np.maximum(var - var * var * Qv.reshape(Ms, -1), 0.0) + noise
    return mean, v


def cube(shape, col_axes, frac, seed=0, axes=None):
    """y on the product grid of `axes` (default: index coordinates) with a fraction of the columns over `col_axes` missing
    along every other axis; X with NaN at the same points."""
    rng = np.random.default_rng(seed)
    axes = axes or [np.arange(n, dtype=np.float64) for n in shape]
    Xg = np.array(np.meshgrid(*axes, indexing="ij"))
    y = np.cos(Xg[0] / 3.0) * np.sin(Xg[1] / 2.0 + 0.3)
    for k in range(2, len(shape)):
        y = y + 0.4 * np.cos(Xg[k] / 2.5 + k)
    y = y + 0.05 * rng.standard_normal(shape)
    cshape = [shape[i] for i in col_axes]
    ncol = int(np.prod(cshape))
    gone = rng.choice(ncol, size=int(round(frac * ncol)), replace=False)
    mask = np.zeros(ncol, dtype=bool)
    mask[gone] = True
    full = [1] * len(shape)
    for i in col_axes:
        full[i] = shape[i]
    mask = np.broadcast_to(mask.reshape(cshape).reshape(full), shape)
    X, y = Xg.copy(), y.copy()
    X[:, mask] = np.nan
    y[mask] = np.nan
    return Xg, X, y
