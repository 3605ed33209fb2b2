"""
smgpr.py -- the spectral-mixture kernel of ``skreconstructor(kernel='Spectral')``: an exact GP on the observed points.

Takes the ROLE of the reference's Spectral branch of gpim/gpreg/skgpr.py (lines 122-164, 209-220, 431-434: no SKI, GPyTorch's
SpectralMixtureKernel, ConstantMean and GaussianLikelihood, initialised by ``initialize_from_data``).  The covariance, the
gradient contraction and the Adam step are HIP launches of the MI355X engine (csrc/sm.hip; include/gpimhip.h:
gpimhip_fit_sm / gpimhip_predict_sm); the factorisation, K^-1 and the solves are the engine's exact-GP path.

Model (float64), Q mixtures, D = d or 1 (isotropic), tau = x_i - x_j:
    k_q(tau) = exp(-2 pi^2 sum_d tau_d^2 s_qd^2) prod_d cos(2 pi tau_d m_qd),   K = sum_q w_q k_q + noise I
    w, m, s = softplus(raw), noise = 1e-4 + softplus(r_n), constant mean c
    u = [c | r_w (Q) | r_m (Q x D) | r_s (Q x D) | r_n]

Readings and deliberate differences, in one place:
  * GPyTorch is not available to check these readings against; they follow GPyTorch's documented semantics.
  * Initialisation (``initial_raw``) restates ``SpectralMixtureKernel.initialize_from_data(X, y)`` in float64 on the CPU
    generator right after ``torch.manual_seed(seed)`` -- the reference's first random draws: per dimension max_dist = the
    range of X and min_dist = the smallest nonzero gap between sorted coordinates; s = 1 / |randn(Q, 1, D) max_dist|,
    m = rand(Q, 1, D) 0.5 / min_dist, w = std(y) / Q (unbiased); raw values log(expm1(x)); c = 0, r_n = 0.  Isotropic
    (D = 1): the largest range and the smallest gap over all dimensions (GPyTorch does not define that case cleanly).
    With ``use_gpu`` the reference draws on the CUDA default tensor type, i.e. from another generator: its numbers can
    differ from these.
  * For N > 800 GPyTorch switches to CG / Lanczos for the solves and log-determinant, and ``fast_pred_var`` approximates
    the predictive variance.  This engine is exact in both.
  * ``num_batches``, ``max_root`` / ``maxroot``, ``grid_points_ratio``, ``ski`` and ``sparse`` are accepted and ignored;
    ``precision='single'`` raises NotImplementedError.
  * ``sample`` (joint posterior draws; the reference has none for this model) is this engine's: DESIGN.md section 24.
  * Solver (``rec.solver``; ``solver='dense' | 'reflection' | 'border'`` forces one): the kernel is stationary and even in
    every coordinate difference, so on a complete product grid with a symmetric axis the model runs as the 2^r reflection
    blocks of N / 2^r points ('reflection'), and on a grid with few missing pixels as the same blocks plus a border
    ('border', chosen by the flop model of gprutils.border_flops against skgpr.BORDER_FACTOR) -- the same model to
    rounding.  Everything else is the dense exact GP on the observed points ('dense').
"""
import ctypes

import numpy as np
import torch

from . import _lib
from . import _sampling, _solvers
from . import gprutils
from ._solvers import HostDriver, SpectralBlocks

_F64 = torch.float64


def _softplus(x):
    x = np.asarray(x, dtype=np.float64)
    return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))


def raw_layout(Q, D):
    """Offsets of u = [c | r_w (Q) | r_m (Q x D) | r_s (Q x D) | r_n] (include/gpimhip.h): dict of slices, and P."""
    o = {"c": slice(0, 1), "w": slice(1, 1 + Q), "m": slice(1 + Q, 1 + Q + Q * D),
         "s": slice(1 + Q + Q * D, 1 + Q + 2 * Q * D), "noise": slice(1 + Q + 2 * Q * D, 2 + Q + 2 * Q * D)}
    return o, 2 + Q * (2 * D + 1)


def constrained(u, Q, D):
    """(c, w (Q,), m (Q, D), s (Q, D), noise) from the raw vector u (numpy float64)."""
    u = np.asarray(u, dtype=np.float64)
    o, _ = raw_layout(Q, D)
    return (float(u[0]), _softplus(u[o["w"]]), _softplus(u[o["m"]]).reshape(Q, D), _softplus(u[o["s"]]).reshape(Q, D),
            float(1e-4 + _softplus(u[o["noise"]])[0]))


def initial_raw(X, y, Q=4, isotropic=False, seed=0):
    """GPyTorch's SpectralMixtureKernel.initialize_from_data(X, y) in float64 after torch.manual_seed(seed) (module
    docstring); X: (N, d) points, y: (N,) targets.  Returns the raw vector u (numpy float64, P entries)."""
    X = torch.as_tensor(np.asarray(X, dtype=np.float64))
    y = torch.as_tensor(np.asarray(y, dtype=np.float64)).reshape(-1)
    d = X.shape[1]
    D = 1 if isotropic else d
    xs = X.sort(dim=0)[0]
    max_dist = xs[-1] - xs[0]
    gaps = xs[1:] - xs[:-1]
    min_dist = torch.stack([gaps[:, k][gaps[:, k] != 0].min() for k in range(d)])
    if isotropic:
        max_dist, min_dist = max_dist.max().reshape(1), min_dist.min().reshape(1)
    torch.manual_seed(seed)
    scales = torch.randn(Q, 1, D, dtype=_F64).mul(max_dist).abs().reciprocal()
    means = torch.rand(Q, 1, D, dtype=_F64).mul(0.5).div(min_dist)
    weights = y.std().div(Q).expand(Q)

    def inv_softplus(v):
        return torch.log(torch.expm1(v))

    _, P = raw_layout(Q, D)
    u = torch.zeros(P, dtype=_F64)
    o, _ = raw_layout(Q, D)
    u[o["w"]] = inv_softplus(weights)
    u[o["m"]] = inv_softplus(means).reshape(-1)
    u[o["s"]] = inv_softplus(scales).reshape(-1)
    return u.numpy()


class smreconstructor(HostDriver):
    """``skreconstructor(X, y, Xtest, kernel='Spectral', ...)`` -- argument order and defaults of gpim/gpreg/skgpr.py:79-91.
    X: (c, *dims) grid coordinates (NaN rows dropped together with the NaN entries of y: sparse images are fine);
    ``n_mixtures`` (default 4) and ``isotropic`` as in the reference.  ``lengthscale`` is not used by this kernel.
    ``solver=None | 'dense' | 'reflection' | 'border'`` forces a solver (module docstring); ``rec.solver`` reports it."""

    def __init__(self, X, y, Xtest=None, kernel='Spectral', lengthscale=None, ski=True, learning_rate=.1,
                 iterations=50, use_gpu=1, verbose=1, seed=0, **kwargs):
        self.precision = kwargs.get("precision", "double")
        if self.precision == "single":
            raise NotImplementedError("skreconstructor(kernel='Spectral'): precision='single' is not implemented by the "
                                      "MI355X engine (the spectral-mixture path runs in double precision)")
        self.objective = _solvers.check_objective(kwargs.get("objective", "nll"))
        if self.objective == "loo":
            _solvers.refuse_loo_objective("spectral-mixture GP (kernel='Spectral')",
                                          "its gradient contraction has a kernel and a constant mean of its own (csrc/sm.hip), "
                                          "for which the leave-one-out form is not built")
        self._handle = _lib.Handle()
        self._dev = self._handle.device
        self.fulldims = Xtest.shape[1:] if Xtest is not None else X.shape[1:]
        Xt, yt = gprutils.prepare_training_data(X, y)
        if Xt.shape[0] != yt.shape[0]:
            raise ValueError("skreconstructor: %d input points but %d observations (NaN patterns of X and y differ)"
                             % (Xt.shape[0], yt.shape[0]))
        self.X, self.y = Xt, yt
        self.Xtest = gprutils.prepare_test_data(Xtest) if Xtest is not None else None
        d = int(Xt.shape[1])
        Q = kwargs.get("n_mixtures") or 4
        if not 1 <= Q <= _lib.SM_MAX_MIXTURES:
            raise ValueError("skreconstructor: n_mixtures must be 1 .. %d (got %r)" % (_lib.SM_MAX_MIXTURES, Q))
        self.isotropic = bool(kwargs.get("isotropic"))
        self.num_mixtures, self._D = int(Q), 1 if self.isotropic else d
        sm = _lib.SmStruct()
        sm.dim, sm.mixtures, sm.ard = d, self.num_mixtures, 0 if self.isotropic else 1
        self._sstruct = sm
        u = initial_raw(Xt.numpy(), yt.numpy(), self.num_mixtures, self.isotropic, seed)
        self._u = torch.from_numpy(u).to(self._dev)
        S, self.solver = self._choose_solver(X, y, kwargs.get("solver"))
        self._solver = None if S is None else SpectralBlocks(S, border=self.solver == "border")
        self._Xd = self._to_device(self.X)
        self._yd = self._to_device(self.y)
        self._Xtest_d = self._to_device(self.Xtest) if self.Xtest is not None else None
        self._draw_bytes = {}        # method -> the largest sample() call that has run (_sampling.reserve)
        self.iterations = iterations
        self.learning_rate = learning_rate
        self.scales, self.means, self.weights, self.noise_all = [], [], [], []
        self.loss_all = []
        self.hyperparams = {"scales": self.scales, "means": self.means, "weights": self.weights,
                            "noise": self.noise_all, "maxdim": max(self.fulldims)}
        self.verbose = verbose

    # ------------------------------------------------------------------ solver choice (host only)
    @staticmethod
    def _reflection_blocks(X, y):
        """The blocks dict of a complete product grid with a symmetric axis (gprutils.reflection_blocks_multi with one task:
        ys (B, Nq) and ones = U 1), else None."""
        X = np.asarray(X, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        if np.isnan(y).any() or np.isnan(X).any() or X.shape[1:] != y.shape:
            return None
        try:
            axes, _ = gprutils.grid_axes(X)
            S = gprutils.reflection_blocks_multi(X, y[..., None], axes)
        except (NotImplementedError, ValueError):
            return None
        S["ys"] = S["ys"][0]
        return S

    @staticmethod
    def _border_blocks(X, y):
        """The blocks dict of an incomplete grid that can be completed and has a symmetric axis (gprutils.border_blocks_multi
        with one task: ys with 0 at the missing points, ones = U 1_o, n_total = the observations), else None."""
        X = np.asarray(X, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        if not np.isnan(y).any():
            return None
        try:
            S = gprutils.border_blocks_multi(X, y[..., None])
        except (NotImplementedError, ValueError):
            return None
        S["ys"] = S["ys"][0]
        S["n_total"] = S["n_obs"]           # the loss is that of the observed points
        return S

    @classmethod
    def _choose_solver(cls, X, y, forced=None):
        """(blocks dict or None, 'dense' | 'reflection' | 'border'): 'reflection' on a complete product grid with at least one
        symmetric axis; 'border' when the grid can be completed and the border's flop model is below skgpr.BORDER_FACTOR of
        the dense model's; else 'dense' (scattered points, no symmetric axis, too many holes).  ``forced`` names a solver and
        raises NotImplementedError when the data do not allow it."""
        from .skgpr import BORDER_FACTOR
        if forced not in (None, "dense", "reflection", "border"):
            raise ValueError("skreconstructor(kernel='Spectral'): solver must be None, 'dense', 'reflection' or 'border' "
                             "(got %r)" % (forced,))
        if forced == "dense":
            return None, "dense"
        if forced == "reflection":
            S = cls._reflection_blocks(X, y)
            if S is None:
                raise NotImplementedError("skreconstructor(kernel='Spectral'): solver='reflection' needs a complete product "
                                          "grid (no NaN) with at least one symmetric axis")
            return S, "reflection"
        if forced == "border":
            S = cls._border_blocks(X, y)
            if S is None:
                raise NotImplementedError("skreconstructor(kernel='Spectral'): solver='border' needs a product grid with "
                                          "missing pixels (NaN in y and in the coordinates), an observation at every index of "
                                          "every axis, and at least one symmetric axis")
            return S, "border"
        S = cls._reflection_blocks(X, y)
        if S is not None:
            return S, "reflection"
        S = cls._border_blocks(X, y)
        if S is not None:
            f_border, f_dense = gprutils.border_flops(S["n_obs"] + len(S["miss"]), len(S["miss"]), len(S["dims"]))
            if f_border < BORDER_FACTOR * f_dense:
                return S, "border"
        return None, "dense"

    # ------------------------------------------------------------------ parameters
    def _params(self):
        return constrained(self._u.cpu().numpy(), self.num_mixtures, self._D)

    def nll_grad(self, u=None):
        """Loss and gradient at the raw vector u (default: the current one) -- the engine's evaluation, for checks."""
        u = self._u if u is None else torch.as_tensor(np.asarray(u, dtype=np.float64)).to(self._dev).contiguous()
        loss = torch.empty(1, dtype=_F64, device=self._dev)
        grad = torch.empty(u.numel(), dtype=_F64, device=self._dev)
        if self._solver is not None:
            _lib.check(self._solver.nll_grad(self, u, loss, grad))
        else:
            _lib.check(self._handle.lib.gpimhip_sm_nll_grad(
                self._handle.h, ctypes.byref(self._sstruct), _lib.ptr(self._Xd), _lib.ptr(self._yd), self._Xd.shape[0],
                _lib.ptr(u), _lib.ptr(loss), _lib.ptr(grad)))
        return float(loss.item()), grad.cpu().numpy()

    # ------------------------------------------------------------------ training (HostDriver.train)
    def _hist_width(self):
        return raw_layout(self.num_mixtures, self._D)[1]

    def _fit(self, T, hist, loss):
        if self._solver is not None:
            return self._solver.fit(self, float(self.learning_rate), T, hist, loss)
        return self._handle.lib.gpimhip_fit_sm(
            self._handle.h, ctypes.byref(self._sstruct), _lib.ptr(self._Xd), _lib.ptr(self._yd), self._Xd.shape[0],
            _lib.ptr(self._u), float(self.learning_rate), T, _lib.ptr(hist), _lib.ptr(loss))

    def _record(self, i, row, loss_i, show):
        Q, D = self.num_mixtures, self._D
        o, _ = raw_layout(Q, D)
        self.weights.append(row[o["w"]].copy())
        self.scales.append((1.0 / np.sqrt(row[o["s"]])).reshape(Q, 1, D))
        self.means.append((1.0 / row[o["m"]]).reshape(Q, 1, D))
        self.noise_all.append(float(row[o["noise"]][0]))
        self.loss_all.append(float(loss_i))
        if show:
            return ('noise: {} ...'.format(np.around(self.noise_all[-1], 7)),)

    def _print_final(self, T):
        if T > 0:
            print('Final parameter values:\n', 'weights: {}'.format(np.around(self.weights[-1], 4)),
                  'noise: {}'.format(np.around(self.noise_all[-1], 7)))

    # ------------------------------------------------------------------ prediction
    def _to_device(self, t):
        if isinstance(t, np.ndarray):
            t = torch.from_numpy(t)
        return t.detach().to(self._dev, _F64).contiguous()

    def _new_test_grid(self, Xtest):
        self.fulldims = (self.X.shape[0],) if Xtest is None else Xtest.shape[1:]
        self._Xtest_d = self._Xd if Xtest is None else self._to_device(self.Xtest)

    def _posterior(self):
        Xs = self._Xtest_d              # (Reflection.predict_grid: the training grid itself takes the mirrored-variance path)
        M = Xs.shape[0]
        mean = torch.empty(M, dtype=_F64, device=self._dev)
        var = torch.empty(M, dtype=_F64, device=self._dev)
        if self._solver is not None:
            _lib.check(self._solver.predict_grid(self, mean, var))
            return mean, var
        _lib.check(self._handle.lib.gpimhip_predict_sm(
            self._handle.h, ctypes.byref(self._sstruct), _lib.ptr(self._Xd), _lib.ptr(self._yd), self._Xd.shape[0],
            _lib.ptr(self._u), _lib.ptr(Xs), M, _lib.ptr(mean), _lib.ptr(var)))
        return mean, var

    def predict(self, Xtest=None, **kwargs):
        """Exact predictive mean and standard deviation of likelihood(model(Xtest)) (noise included), shape fulldims."""
        return self._predict_host(Xtest, kwargs, self._posterior)[:2]

    # ------------------------------------------------------------------ joint posterior draws (_sampling.py)
    _SAMPLE_BUILT = ("skreconstructor(kernel='Spectral').sample: method=%r is not built for the spectral-mixture model; built "
                     "are 'joint' (any finite test rows), 'pathwise' (a complete product test grid with a symmetric axis "
                     "that holds every training row) and 'blocks' (an observation on every point of that grid)")

    def _draw_z(self, n_samples, W, seed=None):
        g = None if seed is None else torch.Generator(self._dev).manual_seed(int(seed))
        return torch.randn((n_samples, W), dtype=_F64, device=self._dev, generator=g)

    def _draw_head(self):
        """The leading arguments of the draw entries.  They run outside reflection mode: the block solvers hold that mode
        only inside ``Reflection._mode``, and a draw depends on the observed rows and u alone."""
        return self._handle.h, ctypes.byref(self._sstruct)

    def _grid_args(self, P):
        d = self._Xd.shape[1]
        return (ctypes.c_int32 * d)(*[int(n) for n in P["shape"]]), int(P["mask"]), (ctypes.c_double * 4)(*P["twoc"])

    def _draw_joint(self, Xs, z, noiseless, jitter, mean, var, out):
        return self._handle.lib.gpimhip_sample_sm(*self._draw_head(), _lib.ptr(self._Xd), _lib.ptr(self._yd), self._Xd.shape[0],
                                                  _lib.ptr(self._u), _lib.ptr(Xs), Xs.shape[0], _lib.ptr(z), z.shape[0],
                                                  int(bool(noiseless)), float(jitter), _lib.ptr(mean), _lib.ptr(var),
                                                  _lib.ptr(out))

    def _draw_pathwise(self, Xs, P, idx, z, noiseless, jitter, mean, out):
        return self._handle.lib.gpimhip_sample_sm_pathwise(*self._draw_head(), _lib.ptr(Xs), *self._grid_args(P),
                                                           ctypes.c_void_p(idx.data_ptr()), _lib.ptr(self._yd),
                                                           self._Xd.shape[0], _lib.ptr(self._u), _lib.ptr(z), z.shape[0],
                                                           int(bool(noiseless)), float(jitter), _lib.ptr(mean), _lib.ptr(out))

    def _draw_blocks(self, Xs, P, z, noiseless, jitter, mean, out):
        y = self._yd
        if P["idx_d"] is not None:      # the observations in grid order
            y = torch.empty_like(self._yd)
            y[P["idx_d"]] = self._yd
        return self._handle.lib.gpimhip_sample_sm_blocks(*self._draw_head(), _lib.ptr(Xs), *self._grid_args(P), _lib.ptr(y),
                                                         _lib.ptr(self._u), _lib.ptr(z), z.shape[0], int(bool(noiseless)),
                                                         float(jitter), _lib.ptr(mean), _lib.ptr(out))

    def sample(self, n_samples=1, Xtest=None, noiseless=False, seed=None, z=None, jitter=None, method='joint'):
        """Joint draws from the posterior on the test grid: ndarray of shape ``(n_samples, *grid shape)``, each slice one
        plausible reconstruction.  Meaning, the layout of ``z`` and the seeding are those of ``reconstructor.sample``; the
        constant mean is part of every draw.  A method is open to every ``rec.solver`` (the posterior depends on the
        observed rows and the parameters only) and gated by the data:

        ``'joint'``: any finite test rows; one factorisation of order N + M; ``z`` is ``(n_samples, M)``; ``jitter >= 0``.
        ``'pathwise'`` (Matheron's rule): a complete product test grid with a symmetric axis that holds every training row
        -- the completed image of a model with missing pixels -- at two factorisations of order M / 2^r and N; ``z`` is
        ``(n_samples, M + N)`` if noiseless, else ``(n_samples, 2 M + N)``, split ``[z_p | z_e | z_n]``.
        ``'blocks'``: an observation on every point of that grid; 2 x 2^r factorisations of order M / 2^r; ``z`` is
        ``(n_samples, 2 M)`` if noiseless, else ``(n_samples, 3 M)``.
        ``jitter`` defaults to 1e-5; the model has no jitter of its own, so 0 < jitter <= noise for ``'pathwise'`` and
        ``'blocks'``.  ``'border'``, ``'kron'`` and ``'columns'`` are not built for this model (NotImplementedError)."""
        if method in ("border", "kron", "columns"):
            raise NotImplementedError(self._SAMPLE_BUILT % (method,))
        if method not in _sampling.SPECTRAL_METHODS:
            raise ValueError("method must be 'joint', 'pathwise' or 'blocks'; got %r" % (method,))
        return _sampling.draw(self, method, n_samples, Xtest, noiseless, seed, z, jitter, _sampling.SPECTRAL_METHODS)
