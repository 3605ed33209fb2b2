"""
Second CPU reference of the structured (Kronecker) exact GP, numpy only: K_i from the exact coordinate differences,
``numpy.linalg.eigh`` per axis, and the loss, gradient and posterior of the dense oracle (oracle/gpim_oracle.py: ExactGP)
written in the eigenbasis Q = (x) Q_i, D = s2 (x) lam_i + jitter + noise.

Why a second one: at axes of several hundred points the dense oracle is no longer good to the 1e-11 that
tests/test_gpu_kron.py asks of the loss at small sizes -- its squared distance is the GEMM form |a|^2 - 2 a.b + |b|^2, which
cancels at coordinates near 1000 -- so a bar for the device at these sizes has to come from how far two CPU evaluations in
double precision are apart.  ``DISTANCES`` records that for every large case; tests/test_kron_host.py holds the two
references to it (x 2) without a GPU, tests/test_gpu_kron.py gives the device 10 x it (or the small-size bar, whichever is
larger).

The table is reproduced by        python tests/kron_oracle.py        (a few seconds).
"""
import math

import numpy as np

TINY, EPS = np.finfo(np.float64).tiny, np.finfo(np.float64).eps
AMP = (1e-4, 10.0)
JITTER = 1e-5

# (shape, u_noise): the axis orders whose eigen-problems run in the <4,2>, <8,1> and streamed instantiations of
# kron_eigh_kernel ((300, 4): 150 + 150; (600, 2): 300 + 300; (1030, 1): 515 + 515) and the <2,4> one ((130, 9): 65 + 65);
# u_noise = -9 takes the noise (e^-9 ~ 1.2e-4) off the small eigenvalues, which e^-2.5 hides
BIG_CASES = (((300, 4), -2.5), ((600, 2), -2.5), ((1030, 1), -2.5), ((130, 9), -2.5), ((600, 2), -9.0))
LS_BOUNDS = (0.7, 9.0)

# |dense oracle - this module| as measured by `python tests/kron_oracle.py`: the loss relative to the loss, the gradient
# per component (u_var, u_ls[0], u_ls[1], u_noise) in absolute terms, mean and variance as the largest absolute difference
# over the test grid of predict_axes()
DISTANCES = {
    ((300, 4), -2.5): {"loss_rel": 1.1e-12, "grad_abs": (3.6e-11, 3.3e-09, 1.0e-09, 5.8e-10), "mean_abs": 9.3e-11, "var_abs": 1.2e-10},
    ((600, 2), -2.5): {"loss_rel": 3.4e-12, "grad_abs": (2.8e-10, 1.1e-09, 9.0e-10, 3.6e-09), "mean_abs": 2.1e-10, "var_abs": 7.9e-10},
    ((1030, 1), -2.5): {"loss_rel": 1.0e-11, "grad_abs": (8.5e-10, 2.1e-08, 0.0e+00, 9.9e-09), "mean_abs": 2.4e-10, "var_abs": 7.9e-10},
    ((130, 9), -2.5): {"loss_rel": 4.6e-13, "grad_abs": (8.7e-12, 3.7e-11, 8.0e-13, 9.5e-11), "mean_abs": 9.5e-12, "var_abs": 2.2e-11},
    ((600, 2), -9.0): {"loss_rel": 2.9e-11, "grad_abs": (1.1e-08, 2.8e-05, 2.0e-08, 4.6e-08), "mean_abs": 6.0e-09, "var_abs": 9.8e-10},
}
# the small-size bars of tests/test_gpu_kron.py, which the large cases never go below
LOSS_RTOL, GRAD_RTOL, GRAD_ATOL, POST_ATOL = 1e-11, 1e-8, 1e-9, 1e-9
DEVICE_MARGIN = 10.0      # the device is a third double-precision evaluation whose rounding differs in kind from both


def device_bars(shape, u_noise, loss_ref, g_ref):
    """(loss atol, gradient atol per component, mean atol, variance atol) for the device against the dense oracle:
    the larger of the small-size bar and DEVICE_MARGIN x the recorded distance of the two CPU references"""
    r = DISTANCES[(tuple(shape), u_noise)]
    g_ref = np.asarray(g_ref, dtype=np.float64)
    small_g = GRAD_RTOL * np.abs(g_ref) + GRAD_ATOL * max(1.0, float(np.abs(g_ref).max()))
    return (max(LOSS_RTOL, DEVICE_MARGIN * r["loss_rel"]) * abs(loss_ref),
            np.maximum(small_g, DEVICE_MARGIN * np.asarray(r["grad_abs"])),
            max(POST_ATOL, DEVICE_MARGIN * r["mean_abs"]), max(POST_ATOL, DEVICE_MARGIN * r["var_abs"]))


def smooth_grid(shape, seed):
    rng = np.random.default_rng(seed)
    idx = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    f = np.ones(shape)
    for k, g in enumerate(idx):
        f = f * np.cos(g / (2.0 + k) + 0.3 * k)
    return f + 0.05 * rng.standard_normal(shape)


def predict_axes(shape):
    """a product test grid of a few thousand points off the training grid: at most 513 points on an axis"""
    return [np.linspace(-0.5, n - 0.5, min(2 * n + 1, 513)) for n in shape]


def _sigmoid(u):
    return np.clip(1.0 / (1.0 + np.exp(-u)), TINY, 1.0 - EPS)


def theta(u, ls_lo, ls_hi, amp=AMP):
    """(var, ls[n_ls], noise) and their derivatives with respect to u = (u_var, u_ls[n_ls], u_noise)"""
    u = np.asarray(u, dtype=np.float64)
    ls_lo, ls_hi = np.atleast_1d(np.asarray(ls_lo, np.float64)), np.atleast_1d(np.asarray(ls_hi, np.float64))
    s = _sigmoid(u[:-1])
    ds = s * (1.0 - s)
    var, dvar = amp[0] + (amp[1] - amp[0]) * s[0], (amp[1] - amp[0]) * ds[0]
    ls, dls = ls_lo + (ls_hi - ls_lo) * s[1:], (ls_hi - ls_lo) * ds[1:]
    noise = math.exp(u[-1])
    return (var, ls, noise), (dvar, dls, noise)


def _mode(T, M, i):
    """M along mode i of the tensor T: out[.., a, ..] = sum_b M[a, b] T[.., b, ..]"""
    return np.moveaxis(np.tensordot(M, T, axes=(1, i)), 0, i)


def _outer(vs):
    out = np.ones(())
    for v in vs:
        out = np.multiply.outer(out, v)
    return out


class KronGP:
    """The model of O.ExactGP on the product grid of ``axes`` with observations ``Y`` (an array of the grid's shape)."""

    def __init__(self, axes, Y, u, ls_lo, ls_hi, jitter=JITTER, amp=AMP):
        self.axes = [np.asarray(a, dtype=np.float64) for a in axes]
        self.d = len(self.axes)
        self.Y = np.asarray(Y, dtype=np.float64).reshape([len(a) for a in self.axes])
        (self.var, ls, self.noise), (self.dvar, dls, self.dnoise) = theta(u, ls_lo, ls_hi, amp)
        self.n_ls = len(ls)
        self.ls = np.broadcast_to(ls, (self.d,)) if self.n_ls == 1 else ls
        self.dls = np.broadcast_to(dls, (self.d,)) if self.n_ls == 1 else dls
        self.sigma = jitter + self.noise
        self.prior = math.log(amp[1] - amp[0]) + float(np.log(np.atleast_1d(ls_hi) - np.atleast_1d(ls_lo)).sum())
        self.lam, self.Q, self.R2 = [], [], []
        for c, l in zip(self.axes, self.ls):
            r2 = ((c[:, None] - c[None, :]) / l) ** 2
            lam, Q = np.linalg.eigh(np.exp(-0.5 * r2))
            self.lam.append(lam); self.Q.append(Q); self.R2.append(r2)
        Yt = self.Y
        for i, Q in enumerate(self.Q):
            Yt = _mode(Yt, Q.T, i)
        self.Lam = _outer(self.lam)
        self.D = self.var * self.Lam + self.sigma
        self.At = Yt / self.D
        self.Yt = Yt

    def loss_and_grad(self):
        """(loss, dloss/du) in the oracle's order u_var, u_ls[...], u_noise"""
        D, At, N = self.D, self.At, self.Y.size
        loss = 0.5 * (self.Yt * At).sum() + 0.5 * np.log(D).sum() + 0.5 * N * math.log(2 * math.pi) + self.prior
        g_var = 0.5 * (self.Lam / D).sum() - 0.5 * (At * At * self.Lam).sum()
        g_noise = 0.5 * (1.0 / D).sum() - 0.5 * (At * At).sum()
        g_ls = np.zeros(self.d)
        for i in range(self.d):
            K = np.exp(-0.5 * self.R2[i])
            Mi = self.Q[i].T @ (K * self.R2[i]) @ self.Q[i]           # Q^T (l dK/dl) Q
            excl = _outer([np.ones_like(l) if k == i else l for k, l in enumerate(self.lam)])
            tr = (_outer([np.diag(Mi) if k == i else l for k, l in enumerate(self.lam)]) / D).sum()
            quad = (At * excl * _mode(At, Mi, i)).sum()
            g_ls[i] = 0.5 * self.var * (tr - quad) / self.ls[i]
        gl = g_ls * self.dls
        gl = np.array([gl.sum()]) if self.n_ls == 1 else gl
        return loss, np.concatenate([[g_var * self.dvar], gl, [g_noise * self.dnoise]])

    def predict(self, taxes):
        """(mean, variance with the noise) on the product grid of the axes taxes, flattened in grid order"""
        mean, q = self.At, 1.0 / self.D
        for i, (t, c, l, Q) in enumerate(zip(taxes, self.axes, self.ls, self.Q)):
            t = np.asarray(t, dtype=np.float64)
            B = np.exp(-0.5 * ((t[:, None] - c[None, :]) / l) ** 2) @ Q
            mean, q = _mode(mean, B, i), _mode(q, B * B, i)
        return (self.var * mean).ravel(), (np.maximum(self.var - self.var ** 2 * q, 0.0) + self.noise).ravel()


def big_case(shape, u_noise):
    """The inputs of one entry of BIG_CASES, as tests/test_gpu_kron.py builds them: (R, axes, u, ls_lo, ls_hi)"""
    import torch
    from oracle import gpim_oracle as O
    d = len(shape)
    R = smooth_grid(shape, seed=sum(shape))
    torch.manual_seed(2)
    kp = O.KernelParams("RBF", d, [[LS_BOUNDS[0]] * d, [LS_BOUNDS[1]] * d])
    u = np.concatenate([[kp.u_var.item()], kp.u_ls.detach().numpy(), [u_noise]])
    return R, [np.arange(n, dtype=np.float64) for n in shape], u, [LS_BOUNDS[0]] * d, [LS_BOUNDS[1]] * d


def dense_reference(shape, u_noise):
    """loss, gradient, mean and variance (on predict_axes(shape)) of the dense oracle for one entry of BIG_CASES"""
    import torch
    from oracle import gpim_oracle as O
    d = len(shape)
    R, axes, u, lo, hi = big_case(shape, u_noise)
    X = torch.from_numpy(np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, d))
    torch.manual_seed(2)
    kp = O.KernelParams("RBF", d, [lo, hi])
    with torch.no_grad():
        kp.u_noise.fill_(u_noise)
    gp = O.ExactGP(X, torch.from_numpy(R.ravel()), kp, JITTER)
    loss, g = gp.loss_and_grad()
    Xs = torch.from_numpy(np.stack(np.meshgrid(*predict_axes(shape), indexing="ij"), -1).reshape(-1, d))
    mean, var = gp.predict(Xs)
    return loss.item(), g.numpy(), mean.numpy(), var.numpy()


def distances(shape, u_noise):
    """the row of DISTANCES for one entry of BIG_CASES, measured now"""
    R, axes, u, lo, hi = big_case(shape, u_noise)
    gp = KronGP(axes, R, u, lo, hi)
    loss, g = gp.loss_and_grad()
    mean, var = gp.predict(predict_axes(shape))
    l0, g0, m0, v0 = dense_reference(shape, u_noise)
    return {"loss_rel": abs(loss - l0) / abs(l0), "grad_abs": tuple(np.abs(g - g0)),
            "mean_abs": float(np.abs(mean - m0).max()), "var_abs": float(np.abs(var - v0).max())}


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    torch.set_num_threads(1)       # as tests/conftest.py does: the oracle's reductions depend on the thread count
    print("DISTANCES = {")
    for shape, un in BIG_CASES:
        r = distances(shape, un)
        print('    (%r, %r): {"loss_rel": %.1e, "grad_abs": (%s), "mean_abs": %.1e, "var_abs": %.1e},'
              % (shape, un, r["loss_rel"], ", ".join("%.1e" % v for v in r["grad_abs"]), r["mean_abs"], r["var_abs"]))
    print("}")
