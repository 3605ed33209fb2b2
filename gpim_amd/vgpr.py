"""
vgpr.py -- ``vreconstructor``: exact GP regression of vector-valued functions (several outputs on one set of inputs).

Same constructor, methods and return values as the reference's gpim/gpreg/vgpr.py:19-283 (GPyTorch ExactGP with a
MultitaskKernel, or per-task ScaleKernels when ``independent=True``, and a rank-0 MultitaskGaussianLikelihood); the
covariance C = B (x) K + diag(s) (x) I of the T tasks is split exactly into T single-task blocks that the MI355X engine
factors in lock-step (include/gpimhip.h: gpimhip_fit_vgp / gpimhip_predict_vgp).

Readings and deliberate differences, in one place:
  * The IndexKernel factor F (T x 1) is drawn as ``torch.randn(T, 1)`` in float64 on the CPU generator right after
    ``torch.manual_seed(seed)`` -- the reference's first random draw.  With ``use_gpu`` the reference draws on the CUDA
    default tensor type, i.e. from another generator: its numbers can differ from these.
  * Independent model: the reference sets ``kernel.batch_shape`` after the kernel is built, which does not reshape
    ``raw_lengthscale``; the lengthscales are therefore shared by all tasks and only the output scales are per task.
    GPyTorch is not available to check this reading against.
  * The loss is -log N(vec Y | mu (x) 1, C) / (N T), GPyTorch's current ExactMarginalLogLikelihood; older GPyTorch
    versions (the reference notebook's) divided by a smaller number.  Adam is invariant to the divisor up to its eps.
  * Prediction returns the EXACT predictive mean and standard deviation of ``likelihood(model(Xtest))`` (noise
    included) -- what the reference estimates from 100 ``rsample`` draws (vgpr.py:213-221; its sd carries a Monte-Carlo
    error of roughly 7 %).  ``n_samples``, ``num_batches`` and ``max_root`` / ``maxroot`` are accepted and ignored.
  * Matern52 uses the engine's form of the covariance function (csrc/kfun.hpp: r = sqrt(r2 + 1e-12)), which differs from
    GPyTorch's by at most ~2.5e-12 per entry.

Solver (``rec.solver``), chosen from the data alone unless the keyword ``solver`` forces one:
  * 'reflection' when X is a complete product grid (no NaN in y) with at least one axis whose coordinates are symmetric
    about its centre -- each task block then splits further into the 2^r reflection blocks of
    gprutils.reflection_blocks_multi, 1 / 4^r of the dense flops and 1 / 2^r of its memory;
  * 'border' when the grid has missing pixels (rows of y with a NaN output, NaN coordinates in X) but can be completed: the
    reflection blocks of the completed grid plus, per task, an M x M border for the M missing pixels
    (gprutils.border_blocks_multi, csrc/border.hip).  Chosen when the flop model of
    gprutils.border_flops is below skgpr.BORDER_FACTOR of the dense model's and at least VGP_BORDER_MIN_OBS rows are observed;
  * 'dense' for anything else (scattered points, no symmetric axis, an image row or column without any observation, too
    many missing pixels, small grids).
All three compute the same model on the observed rows: the numbers agree to rounding.  ``solver='dense' | 'reflection' |
'border'`` forces one; NotImplementedError if the data do not allow it.
"""
import ctypes

import numpy as np
import torch

from . import _lib, _sampling, _solvers
from . import gprutils
from ._solvers import DeviceBlocks, HostDriver
from .skgpr import BORDER_FACTOR

# Below this many observed rows the border solver is not chosen automatically: the flop model knows neither the padding of
# every block and border to 128 nor the border's extra launches (a 12 x 12 grid with one NaN has a model ratio of 0.066 and
# is one padded tile per block either way).  Measured, not derived: the table of DESIGN.md section 13
# (tests/tools/bench_vgp_border.py --floor).
VGP_BORDER_MIN_OBS = 973

_F64 = torch.float64
_KERNELS = {"RBF": 0, "Matern52": 1}


def _softplus(x):
    x = np.asarray(x, dtype=np.float64)
    return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64)))


def raw_layout(T, n_ls, independent, rank=1):
    """Offsets of u = [mu (T) | F (T x rank) or r_o (T) | r_v (T, correlated only) | r_l (n_ls) | r_a (T) | r_g]
    (include/gpimhip.h): dict of slices, and the length P."""
    o = {"mu": slice(0, T)}
    if independent:
        o["scale"] = slice(T, 2 * T)
        p = 2 * T
    else:
        o["F"] = slice(T, T + T * rank)
        o["rv"] = slice(T + T * rank, 2 * T + T * rank)
        p = 2 * T + T * rank
    o["ls"] = slice(p, p + n_ls)
    o["noise"] = slice(p + n_ls, p + n_ls + T)
    o["global"] = slice(p + n_ls + T, p + n_ls + T + 1)
    return o, p + n_ls + T + 1


def constrained(u, T, n_ls, independent, bounds=None, rank=1):
    """Host restatement of the device maps: (mu, B, s, lengthscales) from the raw vector u (numpy float64)."""
    u = np.asarray(u, dtype=np.float64)
    o, _ = raw_layout(T, n_ls, independent, rank)
    mu = u[o["mu"]].copy()
    if independent:
        B = np.diag(_softplus(u[o["scale"]]))
    else:
        F = u[o["F"]].reshape(T, rank)
        B = F @ F.T + np.diag(_softplus(u[o["rv"]]))
    r = u[o["ls"]]
    if bounds is None:
        ls = _softplus(r)
    else:
        lo, hi = bounds
        ls = _sigmoid(r) * (hi - lo) + lo
    s = (1e-4 + _softplus(u[o["noise"]])) + (1e-4 + _softplus(u[o["global"]][0]))
    return mu, B, s, ls


class vreconstructor(HostDriver):
    """``vreconstructor(X, y, Xtest=None, kernel='RBF', lengthscale=None, independent=False, learning_rate=.1,
    iterations=50, use_gpu=1, verbose=1, seed=0, **kwargs)`` -- argument order and defaults of gpim/gpreg/vgpr.py:73-85.

    X: (c, *dims) grid coordinates; y: (*dims, T) observations of T outputs (rows with a NaN output are dropped);
    kernel: 'RBF' or 'Matern52'; lengthscale: [lower, upper] bounds (two scalars or two lists of c), or None (unbounded,
    softplus); independent: per-task output scales instead of the task covariance.  ``isotropic=True`` gives one
    lengthscale for all dimensions; ``solver=None | 'dense' | 'reflection' | 'border'`` forces a solver (module docstring).
    After training, ``task_covar`` (B), ``noise`` (s), ``mean_constants`` (mu) and
    ``lengthscale`` hold the constrained parameters."""

    def __init__(self, X, y, Xtest=None, kernel='RBF', lengthscale=None, independent=False, learning_rate=.1,
                 iterations=50, use_gpu=1, verbose=1, seed=0, **kwargs):
        self.precision = kwargs.get("precision", "double")
        if self.precision == "single":
            raise NotImplementedError("vreconstructor: precision='single' is not implemented by the MI355X engine "
                                      "(the multi-output GP runs in double precision)")
        if kernel not in _KERNELS:
            raise NotImplementedError("vreconstructor: kernel %r is not implemented by the MI355X engine "
                                      "('RBF' or 'Matern52'; the spectral-mixture kernel is out of scope)" % (kernel,))
        self.objective = _solvers.check_objective(kwargs.get("objective", "nll"))
        if self.objective == "loo":
            _solvers.refuse_loo_objective("multi-output GP (vreconstructor)",
                                          "a held-out point is a vector of T correlated outputs: its predictive density needs "
                                          "the T x T diagonal blocks of S^-1, which the dense engine's scalar diagonal is not")
        self._handle = _lib.Handle()
        self._dev = self._handle.device
        torch.manual_seed(seed)
        input_dim = np.ndim(y) - 1
        Xt, yt = gprutils.prepare_training_data(X, y, vector_valued=True)
        if Xt.shape[0] != yt.shape[0]:
            raise ValueError("vreconstructor: %d input points but %d observation rows (NaN patterns of X and y differ)"
                             % (Xt.shape[0], yt.shape[0]))
        T = int(yt.shape[-1])
        if T > _lib.VGP_MAX_TASKS:
            raise ValueError("vreconstructor: at most %d outputs (got %d)" % (_lib.VGP_MAX_TASKS, T))
        self.num_tasks = T
        self.fulldims = (Xtest.shape[1:] if Xtest is not None else X.shape[1:]) + (T,)
        self.X, self.y = Xt, yt
        self.Xtest = gprutils.prepare_test_data(Xtest) if Xtest is not None else None
        isotropic = bool(kwargs.get("isotropic"))
        self.isotropic = isotropic
        n_ls = 1 if isotropic else input_dim
        self._n_ls = n_ls
        m = _lib.ModelStruct()
        m.kernel, m.dim, m.n_ls = _KERNELS[kernel], input_dim, n_ls
        m.amp_lo, m.amp_hi, m.jitter = 0.0, 1.0, 0.0
        self._bounds = None
        if lengthscale is not None:
            lo = np.broadcast_to(np.asarray(lengthscale[0], dtype=np.float64), (n_ls,)).copy()
            hi = np.broadcast_to(np.asarray(lengthscale[1], dtype=np.float64), (n_ls,)).copy()
            self._bounds = (lo, hi)
            for k in range(n_ls):
                m.ls_lo[k], m.ls_hi[k] = lo[k], hi[k]
        self._mstruct = m
        vg = _lib.VgpStruct()
        vg.tasks, vg.rank, vg.independent, vg.ls_softplus = T, 1, int(bool(independent)), int(lengthscale is None)
        self._vstruct = vg
        self.independent = bool(independent)
        _, P = raw_layout(T, n_ls, self.independent)
        u = torch.zeros(P, dtype=_F64)
        if not self.independent:        # IndexKernel covar_factor = randn(T, 1): the first draw after manual_seed(seed)
            o, _ = raw_layout(T, n_ls, False)
            u[o["F"]] = torch.randn(T, 1, dtype=_F64).reshape(-1)
        self._u = u.to(self._dev)
        self._refl, self.solver = self._choose_solver(X, y, kwargs.get("solver"))
        self._blocks = None
        if self._refl is None:
            self._Xd = self.X.to(self._dev, _F64).contiguous()
            self._Yd = self.y.to(self._dev, _F64).t().contiguous()        # T x N, task-major
        else:       # the fundamental domain, the targets as T x 2^r x N_q, the weights tiled once per task (T 2^r x N_q)
            self._blocks = DeviceBlocks(self._refl, self._dev, tasks=T)
            self._Xd, self._Yd = self._blocks.Xq, self._blocks.ys
            if self.solver == "border":        # the missing pixels' representatives and coefficients, shared by the tasks
                self._blocks.upload_border()
        self.iterations = iterations
        self.learning_rate = learning_rate
        self.lscales = []
        self.loss_all = []
        self.hyperparams = {"lengthscale": self.lscales}
        self.verbose = verbose
        self._draw_bytes = {}           # method -> the largest sample() call that has run (_sampling.reserve)

    @staticmethod
    def _reflection_blocks(X, y):
        """gprutils.reflection_blocks_multi of the data when X (d, n_1, ..., n_d) is a product grid of y's shape, y has no
        NaN and some axis is symmetric; otherwise None (the dense solver)."""
        X = np.asarray(X, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        if np.isnan(y).any() or np.isnan(X).any() or X.shape[1:] != y.shape[:-1]:
            return None
        try:
            axes, _ = gprutils.grid_axes(X)
            return gprutils.reflection_blocks_multi(X, y, axes)
        except (NotImplementedError, ValueError):
            return None

    @staticmethod
    def _border_blocks(X, y):
        """gprutils.border_blocks_multi of the data when y has NaN rows on a grid that can be completed and has a symmetric
        axis; otherwise None."""
        X = np.asarray(X, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        if not np.isnan(y).any():
            return None
        try:
            S = gprutils.border_blocks_multi(X, y)
        except (NotImplementedError, ValueError):
            return None
        S["n_total"] = S["n_obs"]           # the loss is that of the observed rows
        return S

    @classmethod
    def _choose_solver(cls, X, y, forced=None):
        """(blocks or None, 'dense' | 'reflection' | 'border'): the rule of the module docstring."""
        if forced not in (None, "dense", "reflection", "border"):
            raise ValueError("vreconstructor: solver must be None, 'dense', 'reflection' or 'border' (got %r)" % (forced,))
        if forced == "dense":
            return None, "dense"
        if forced == "reflection":
            S = cls._reflection_blocks(X, y)
            if S is None:
                raise NotImplementedError("vreconstructor: solver='reflection' needs a complete product grid (no NaN) with "
                                          "at least one symmetric axis")
            return S, "reflection"
        if forced == "border":
            S = cls._border_blocks(X, y)
            if S is None:
                raise NotImplementedError("vreconstructor: solver='border' needs a product grid with missing pixels (NaN rows "
                                          "of y, NaN coordinates of X), an observation at every index of every axis, and at "
                                          "least one symmetric axis")
            return S, "border"
        S = cls._reflection_blocks(X, y)
        if S is not None:
            return S, "reflection"
        S = cls._border_blocks(X, y)
        if S is not None and S["n_obs"] >= VGP_BORDER_MIN_OBS:
            # the same measured factor as skreconstructor's (the number of tasks cancels out of the ratio)
            f_border, f_dense = gprutils.border_flops(S["n_obs"] + len(S["miss"]), len(S["miss"]), len(S["dims"]))
            if f_border < BORDER_FACTOR * f_dense:
                return S, "border"
        return None, "dense"

    def _engine(self, fn, *args):
        """fn(h, m, vg, X, Y, N, *args) on the handle; in reflection mode (set around this call only) X is the fundamental
        domain and Y the projected targets; the 'border' solver sets the missing pixels as well."""
        call = lambda: fn(self._handle.h, ctypes.byref(self._mstruct), ctypes.byref(self._vstruct), _lib.ptr(self._Xd), _lib.ptr(self._Yd),
                          self._Xd.shape[0], *args)
        if self._blocks is None:
            return call()
        with _lib.reflection(self._handle, self._blocks, border=self._blocks.border):
            return call()

    # ------------------------------------------------------------------ parameters
    def _params(self):
        return constrained(self._u.cpu().numpy(), self.num_tasks, self._n_ls, self.independent, self._bounds)

    @property
    def mean_constants(self):
        return self._params()[0]

    @property
    def task_covar(self):
        return self._params()[1]

    @property
    def noise(self):
        return self._params()[2]

    @property
    def lengthscale(self):
        return self._params()[3]

    def nll_grad(self, u=None):
        """Loss and gradient at the raw vector u (default: the current one) -- the engine's evaluation, for checks."""
        u = self._u if u is None else torch.as_tensor(u, dtype=_F64).to(self._dev).contiguous()
        loss = torch.empty(1, dtype=_F64, device=self._dev)
        grad = torch.empty(u.numel(), dtype=_F64, device=self._dev)
        _lib.check(self._engine(self._handle.lib.gpimhip_vgp_nll_grad, _lib.ptr(u), _lib.ptr(loss), _lib.ptr(grad)))
        return float(loss.item()), grad.cpu().numpy()

    # ------------------------------------------------------------------ training (HostDriver.train)
    def _hist_width(self):
        return self._n_ls

    def _fit(self, T, hist, loss):
        return self._engine(self._handle.lib.gpimhip_fit_vgp, _lib.ptr(self._u), float(self.learning_rate), T, _lib.ptr(hist),
                            _lib.ptr(loss))

    def _record(self, i, row, loss_i, show):
        self.lscales.append(row.tolist())
        self.loss_all.append(float(loss_i))
        if show:
            return ('length: {} ...'.format(np.around(self.lscales[-1], 4)),)

    def _print_final(self, T):
        if T > 0:
            print('Final parameter values:\n',
                  'lengthscale: {}'.format(np.around(self.lscales[-1], 4)))

    # ------------------------------------------------------------------ prediction
    def _new_test_grid(self, Xtest):
        self.fulldims = ((self.X.shape[0],) if Xtest is None else Xtest.shape[1:]) + (self.num_tasks,)

    def _posterior(self):
        Xs = self.Xtest.to(self._dev, _F64).contiguous()
        M = Xs.shape[0]
        mean = torch.empty((M, self.num_tasks), dtype=_F64, device=self._dev)
        var = torch.empty((M, self.num_tasks), dtype=_F64, device=self._dev)
        _lib.check(self._engine(self._handle.lib.gpimhip_predict_vgp, _lib.ptr(self._u), _lib.ptr(Xs), M, _lib.ptr(mean),
                                _lib.ptr(var)))
        return mean, var

    def predict(self, Xtest=None, **kwargs):
        """Exact predictive mean and standard deviation at Xtest, shape ``Xtest.shape[1:] + (T,)`` each."""
        return self._predict_host(Xtest, kwargs, self._posterior)[:2]

    # ------------------------------------------------------------------ joint posterior draws
    _SAMPLE_BUILT = ("vreconstructor.sample: method=%r is not built for the multi-output model; built are 'joint' (any test "
                     "points) and 'blocks' (a fully observed grid with a symmetric axis)")

    def _observed(self):
        """(X (N, d), Y (T, N) task-major) device tensors of the observed rows -- all the posterior depends on besides u.
        The dense solver holds them already; the others upload them at the first draw and keep them."""
        if self._blocks is None:
            return self._Xd, self._Yd
        c = getattr(self, "_obs_d", None)
        if c is None:
            c = self._obs_d = (self.X.to(self._dev, _F64).contiguous(), self.y.to(self._dev, _F64).t().contiguous())
        return c

    def sample(self, n_samples=1, Xtest=None, noiseless=False, seed=None, z=None, jitter=None, method='joint'):
        """Joint draws of all T outputs from the posterior on the test grid: ndarray of shape ``(n_samples,) + grid shape +
        (T,)``, each slice one plausible stack of outputs that vary together as the posterior says.  The block reduction
        makes the posterior of the T whitened, rotated latent functions independent, so a draw is T single-output draws
        mixed back; every ``rec.solver`` draws from the same posterior of the observed rows.
        ``Xtest`` as in ``predict``; the test grid must be finite.  ``noiseless=False`` includes each task's noise.

        ``jitter`` (default 1e-5, > 0) is RELATIVE TO EACH TASK'S NOISE: the covariance of task a's draws carries
        ``noise[a] * jitter`` on its diagonal (the latent blocks have unit noise, and the jitter is theirs).

        ``z``: optional standard normals of shape ``(T, n_samples, W)``, array or device tensor, used as is (the result is
        then a pure function of the model); block t's slice is what the single-output draw of latent block t takes.  When
        absent it is drawn as ``torch.randn((T, n_samples, W), dtype=torch.float64, device=dev, generator=g)`` with
        ``g = torch.Generator(dev).manual_seed(seed)`` (``seed is None``: the global device generator).

        ``method='joint'``: one factorisation of order N + M per latent block, any test points; W = M.
        ``method='blocks'``: for data that fill a product grid (no NaN) with at least one symmetric axis, drawn on that
        grid (``Xtest`` None, the stored grid, or equal to it) through its reflection blocks: 2 x 2^r factorisations of
        order M / 2^r per latent block; W = 2 M if noiseless, else 3 M; jitter <= 1.
        ``'pathwise'`` and ``'border'`` are not built for this model (NotImplementedError)."""
        if method in ("pathwise", "border"):
            raise NotImplementedError(self._SAMPLE_BUILT % (method,))
        if method not in ("joint", "blocks"):
            raise ValueError("method must be 'joint' or 'blocks' ('pathwise' and 'border' are not built for the multi-output "
                             "model); got %r" % (method,))
        S, T = int(n_samples), self.num_tasks
        if S < 1:
            raise ValueError("n_samples must be at least 1; got %r" % (n_samples,))
        jitter = 1e-5 if jitter is None else float(jitter)
        if not (jitter > 0.0) or (method == "blocks" and jitter > 1.0):
            raise ValueError("sample: jitter is relative to each task's noise and must be > 0%s; got %g"
                             % (" and <= 1 for method='blocks'" if method == "blocks" else "", jitter))
        # the test grid, resolved without storing it: a refused call leaves the model as it was
        Xs_h, shape = _sampling.rows_grid(Xtest, gprutils.prepare_test_data, (self.Xtest, tuple(self.fulldims[:-1])),
                                          (self.X, (self.X.shape[0],)))
        if not bool(torch.isfinite(Xs_h).all()):
            raise ValueError(_sampling.FINITE)
        M, N, d = Xs_h.shape[0], self.X.shape[0], self.X.shape[1]
        P = None
        if method == "blocks":
            if len(shape) != d or int(np.prod(shape)) != M:
                raise NotImplementedError("method='blocks' needs a product grid as its test grid: %d test rows do not fill a "
                                          "grid of shape %s in %d dimensions" % (M, shape, d))
            P = gprutils.pathwise_grid(Xs_h.numpy().T.reshape((d,) + shape), self.X.numpy())     # NotImplementedError, with the reason
            if N != M:
                first = int(np.setdiff1d(np.arange(M), P["idx"])[0])
                raise NotImplementedError("method='blocks' needs an observation of all outputs on every point of the test grid "
                                          "(a complete stack, and the test grid must be the training grid): grid point %s has "
                                          "none (%d observed rows, %d grid points)"
                                          % (tuple(int(v) for v in np.unravel_index(first, shape)), N, M))
            W = 2 * M + (0 if noiseless else M)
        else:
            W = M
        if z is None:
            g = None if seed is None else torch.Generator(self._dev).manual_seed(int(seed))
            z_d = torch.randn((T, S, W), dtype=_F64, device=self._dev, generator=g)
        else:
            z_d = (z if torch.is_tensor(z) else torch.from_numpy(np.asarray(z))).to(self._dev, _F64).contiguous()
            if tuple(z_d.shape) != (T, S, W):
                raise ValueError("z must have shape (T, n_samples, W) = (%d, %d, %d) for method=%r (M = %d test points); got %s"
                                 % (T, S, W, method, M, tuple(z_d.shape)))
        # the one large allocation of the call (kept by the handle, grow-only): a single-output call's at the same sizes
        if method == "joint":
            need, what = _sampling.factor_bytes(N + M), "the joint covariance of %d observed rows and %d test points needs" % (N, M)
        else:
            nq = _sampling.block_points(P)
            need, what = _sampling.factor_bytes(nq), "a reflection block of %d points needs" % nq
        _sampling.reserve(self, method, need, what)
        self._resolve_test_grid(Xtest)
        Xo, Yo = self._observed()
        Xs = Xs_h.to(self._dev, _F64).contiguous()
        out = torch.empty((S, M, T), dtype=_F64, device=self._dev)
        lib, head = self._handle.lib, (self._handle.h, ctypes.byref(self._mstruct), ctypes.byref(self._vstruct))
        if method == "joint":
            rc = lib.gpimhip_sample_vgp(*head, _lib.ptr(Xo), _lib.ptr(Yo), N, _lib.ptr(self._u), _lib.ptr(Xs), M, _lib.ptr(z_d), S,
                                        int(bool(noiseless)), jitter, None, None, _lib.ptr(out))
        else:
            Yg = Yo
            if not np.array_equal(P["idx"], np.arange(M)):      # the observed rows in grid order
                Yg = torch.empty_like(Yo)
                Yg[:, torch.from_numpy(P["idx"]).to(self._dev)] = Yo
            cshape = (ctypes.c_int32 * d)(*[int(n) for n in P["shape"]])
            twoc = (ctypes.c_double * 4)(*P["twoc"])
            rc = lib.gpimhip_sample_vgp_blocks(*head, _lib.ptr(Xs), cshape, int(P["mask"]), twoc, _lib.ptr(Yg), _lib.ptr(self._u),
                                               _lib.ptr(z_d), S, int(bool(noiseless)), jitter, None, _lib.ptr(out))
        _lib.check(rc)
        _sampling.record(self, method, need)
        return out.cpu().numpy().reshape((S,) + shape + (T,))
