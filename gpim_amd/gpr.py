"""
gpr.py -- ``reconstructor``: exact Gaussian-process regression on image / hyperspectral grids,
computed by the MI355X engine (libgpimhip.so).

Host-side mirror of the reference's gpim/gpreg/gpr.py:22-283:
same constructor signature, same ``train`` / ``predict`` / ``run`` methods and return values,
same ``hyperparams`` dictionary.  What the reference delegates to pyro.contrib.gp / torch
(kernel matrix, Cholesky, marginal log-likelihood and its gradient, Adam, posterior) runs as
hand-written HIP kernels behind the C ABI of include/gpimhip.h.

Deliberate differences from the reference, all on the outside of the numerics:
  * the engine is GPU-only.  ``use_gpu`` is accepted for signature compatibility and ignored;
    without a HIP device or without libgpimhip.so every call raises RuntimeError.
  * the initial hyper-parameters are always drawn with torch's CPU generator (the reference does
    that on its CPU path; its CUDA path uses the CUDA generator and is not reproducible).
  * no process-global side effects: torch's default tensor type is left alone.
  * a non-positive-definite covariance during training freezes the hyper-parameters, the optimiser
    and the history on the device at the failing iteration (what the reference's state is when
    torch.linalg.cholesky raises, gpr.py:192); the host stops enqueueing a bounded number of
    iterations later and ``train`` raises the same exception class with the history up to that
    iteration appended, so the reconstructor stays usable.
  * ``precision='single'``: inputs are taken, the initial hyper-parameters drawn and the results
    returned in float32 like the reference does, and the exact-GP engine runs in single precision
    (gpimhip_set_precision(h, 32): float N x N matrices, every O(N^3) product on the fp32 matrix
    cores -- 1.7x the double-precision throughput at N = 16384 and half the memory); diagonal blocks,
    the O(N) vectors, loss, gradient and Adam stay double and K^-1 y is refined once against the
    covariance in double, so posterior means are at least as accurate as a float32 run of the reference
    (variances and the loss: float32 round-off times the conditioning), not bit-comparable to one.  Sparse and structured models, and the
    fused trainer for N <= 128, compute in double on either setting.
"""
import random

import numpy as np
import torch

from . import _lib, _solvers, gprutils
from .kernels import get_kernel

_F64 = torch.float64


class _KernelView:
    """``model.kernel`` facade: constrained values as tensors (boptim.py:319 reads
    ``model.kernel.lengthscale.mean().item()``)."""

    def __init__(self, owner):
        self._o = owner

    @property
    def variance(self):
        return self._o._spec.constrained(self._o._u)[0]

    @property
    def lengthscale(self):
        ls = self._o._spec.constrained(self._o._u)[1]
        return ls.reshape(()) if self._o._spec.isotropic else ls

    variance_map = variance
    lengthscale_map = lengthscale


class _ModelView:
    """``reconstructor.model`` facade with settable training data (boptim.py:248-249 swaps
    ``model.X`` / ``model.y`` in place between trainings)."""

    def __init__(self, owner):
        self._o = owner
        self.kernel = _KernelView(owner)

    @property
    def X(self):
        return self._o._Xd

    @X.setter
    def X(self, value):
        self._o._no_swap("X")
        self._o._Xd = self._o._to_device(value)

    @property
    def y(self):
        return self._o._yd

    @y.setter
    def y(self, value):
        self._o._no_swap("y")
        self._o._yd = self._o._to_device(value)

    @property
    def noise(self):
        return self._o._spec.constrained(self._o._u)[2]

    @property
    def jitter(self):
        return self._o._spec.jitter

    @property
    def Xu(self):
        o = self._o
        P = o._spec.n_params
        return o._u[P:].reshape(o._n_ind, o._spec.dim) if o._n_ind else None

    def parameters(self):
        yield self._o._u


class reconstructor(_solvers.HostDriver):
    """
    Gaussian-process reconstruction of sparse 2D images and 3D/4D hyperspectral data.

    Args:
        X (ndarray): grid indices, :math:`c \\times N \\times M (\\times L ...)`; NaN = missing
        y (ndarray): observations, :math:`N \\times M (\\times L ...)`; NaN = missing
        Xtest (ndarray): grid on which to predict (same layout as X)
        kernel (str): 'RBF', 'Matern52' or 'RationalQuadratic'
        lengthscale: ``[lo, hi]`` (one shared lengthscale) or ``[[lo...], [hi...]]`` bounds;
            default ``[[0]*d, [mean(y.shape)/2]*d]``
        sparse (bool), indpoints (int): sparse variational GP (VFE) with trainable inducing inputs, initialised as
            X[::len(X) // indpoints] like the reference (csrc/vfe.hip)
        learning_rate (float), iterations (int): Adam settings
        use_gpu: ignored (always on the GPU)
        verbose (int): 0, 1 or 2
        seed (int): seeds the CPU generator used for the initial hyper-parameter draw
        **amplitude, **precision, **jitter, **isotropic: as in the reference
        **structured (bool): gpim_amd extension -- exact GP through the Kronecker structure of the
            covariance (csrc/kron.hip).  Requires fully observed data on a product grid (X as returned
            by ``utils.get_full_grid``) and the RBF kernel; same model, parameterisation and results as
            the dense path, O(sum n_i^3 + N sum n_i) instead of O(N^3) work.  Takes the role of the
            reference's structured-kernel ``skreconstructor`` (gpim/gpreg/skgpr.py), exact rather than
            interpolated.  With a kernel that does not factorise over the axes ('Matern52', 'RationalQuadratic') the
            reflection symmetry of the complete grid is used instead: in the basis adapted to the reflections of every
            axis the covariance is block diagonal -- 2^r dense blocks of N / 2^r points, one lock-step
            batch with shared hyper-parameters (csrc/engine.hip: kmat_refl_kernel) -- 4^-r of the dense model's O(N^3)
            work (1/16 for a 2-D image), the same model and results to rounding; predictions at arbitrary points.  Axes of
            odd length are reflected too (their mirror plane belongs to the fundamental domain, with weights).
    """

    def __init__(self, X, y, Xtest=None, kernel='RBF', lengthscale=None, sparse=False,
                 indpoints=None, learning_rate=5e-2, iterations=1000, use_gpu=False,
                 verbose=1, seed=0, **kwargs):
        self.precision = kwargs.get("precision", "double")
        self._np_out = np.float32 if self.precision == "single" else np.float64
        # raises if there is no GPU / no library; single precision applies to the exact dense engine only
        single_engine = self.precision == "single" and not sparse and not kwargs.get("structured", False)
        self._handle = _lib.Handle(precision="single" if single_engine else "double")
        self._dev = self._handle.device
        self.verbose = verbose
        # pyro.set_rng_seed(seed) at gpr.py:101 seeds torch, numpy and Python's random: the boptimizer
        # paths that draw from np.random (checkvalues' exit strategy, update_points' padding) depend on it
        torch.manual_seed(seed)
        np.random.seed(seed)
        random.seed(seed)
        input_dim = np.ndim(y)
        self.X, self.y = gprutils.prepare_training_data(X, y, precision=self.precision)
        self._kernel_name = kernel
        structured = bool(kwargs.get("structured", False))
        border = kwargs.get("_border")       # set by skreconstructor on an incomplete grid (gprutils.border_blocks)
        columns = kwargs.get("_columns")     # set by skreconstructor when whole columns are missing (gprutils.column_blocks)
        if structured and columns is not None:
            # J dense blocks of the observed ragged points, one per eigen-direction of the complete axes (csrc/pkron.hip)
            if kernel != "RBF":
                raise NotImplementedError("column blocks: only the RBF kernel factorises over the complete axes")
            self._solver = _solvers.Columns(columns)
        elif structured and border is not None:
            # the reflection blocks of the completed grid with a border for its missing points (csrc/border.hip)
            border["n_total"] = border["n_obs"]          # the loss is that of the observed points
            self._solver = _solvers.Reflection(border, border=True)
        elif structured:
            if sparse:
                raise NotImplementedError("structured=True and sparse=True are mutually exclusive")
            if np.isnan(np.asarray(y)).any():
                raise NotImplementedError("structured=True needs a fully observed grid (no NaN in y)")
            axes, axes_n = gprutils.grid_axes(X)
            if kernel == "RBF":
                self._solver = _solvers.Kron(axes, axes_n)
            else:
                # kernels that do not factorise over the axes (Matern52, RationalQuadratic): the reflection symmetry of the
                # complete grid instead -- 2^r diagonal blocks of N / 2^r points each, r = the axes of even length
                try:
                    S = gprutils.reflection_blocks(np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64), axes)
                except ValueError as e:
                    raise NotImplementedError("structured=True with kernel %r: %s" % (self._kernel_name, e))
                self._solver = _solvers.Reflection(S)
        else:
            self._solver = _solvers.Sparse() if sparse else _solvers.Dense()
        self.do_sparse = bool(sparse)
        self.do_structured, self.do_symm, self.do_border = (self._solver.structured, self._solver.symm, self._solver.border)
        if lengthscale is None:
            lengthscale = gprutils.default_lengthscale(y.shape, kwargs.get("isotropic"))
        self._spec = get_kernel(kernel, input_dim, lengthscale, use_gpu,
                                amplitude=kwargs.get('amplitude'), precision=self.precision,
                                jitter=kwargs.get("jitter", 1.0e-5))
        # drawn from a private generator seeded like the global one: identical numbers, no race when
        # several reconstructors are built from different threads
        self._u = self._spec.draw_initial_u(
            torch.Generator().manual_seed(seed),
            torch.float32 if self.precision == "single" else _F64).to(self._dev)
        self._mstruct = self._spec.struct()
        self._n_ind = 0
        if self.do_sparse:
            # inducing inputs: every (N // indpoints)-th observation, trainable (gpr.py:145-153)
            n = len(self.X)
            Xu = self.X[::n // gprutils.n_inducing(n, indpoints)]
            if self.verbose == 2:
                print("# of inducing points for sparse GP regression: {}".format(len(Xu)))
            self._n_ind = len(Xu)
            self._u = torch.cat([self._u, Xu.reshape(-1).to(self._dev, _F64)]).contiguous()
        self.fulldims = Xtest.shape[1:] if Xtest is not None else X.shape[1:]
        self.Xtest = gprutils.prepare_test_data(Xtest, precision=self.precision) if Xtest is not None else None
        self._Xd = self._to_device(self.X)
        self._yd = self._to_device(self.y)
        self._Xtest_d = self._to_device(self.Xtest) if self.Xtest is not None else None
        self._solver.attach(self)
        if Xtest is not None:
            self._solver.new_test_grid(Xtest)
        self.learning_rate = learning_rate
        self.iterations = iterations
        self.indpoints_all = []
        self.lscales, self.noise_all, self.amp_all = [], [], []
        self.loss_all = []
        self.hyperparams = {
            "lengthscale": self.lscales,
            "noise": self.noise_all,
            "variance": self.amp_all,
            "inducing_points": self.indpoints_all
        }
        self._last_pred = None       # (mean, sd) device tensors of the latest predict()

    @property
    def model(self):
        """The ``model`` facade of the reference object (``model.X`` / ``model.y`` settable, ``model.kernel``).  Built per
        access: a stored view would close a reference cycle with this object, and the library handle -- with its N x N
        workspaces -- would then live until the cyclic collector happens to run (seen as a 50-65 ms hipFree inside the NEXT
        Bayesian-optimisation run's first training, tools/r5_c4_steps.py)."""
        return _ModelView(self)

    # ------------------------------------------------------------------ helpers
    def _no_swap(self, what):
        """structured=True models are built from the complete grid once (coordinate vectors of the Kronecker solver, the
        reflection blocks and projected observations of the symmetry-reduced one): swapping the training data through
        ``model.X`` / ``model.y`` would leave them stale and train / predict on the old observations silently."""
        if self.do_symm or self.do_structured:
            raise NotImplementedError("structured=True: the training data cannot be replaced through model.%s "
                                      "(build a new reconstructor for new observations)" % what)

    def _to_device(self, t):
        if isinstance(t, np.ndarray):
            t = torch.from_numpy(t)
        return t.detach().to(self._dev, _F64).contiguous()

    def _check_data(self):
        X, y = self._Xd, self._yd
        if X.dim() != 2 or X.shape[1] != self._spec.dim or y.dim() != 1 or y.shape[0] != X.shape[0]:
            raise ValueError("training data must be X:(N,%d), y:(N,); got %s and %s"
                             % (self._spec.dim, tuple(X.shape), tuple(y.shape)))
        if X.shape[0] < 1:
            raise ValueError("no observations (all NaN)")

    # ------------------------------------------------------------------ training (HostDriver.train)
    _print_every, _avg_time_above = 100, 0
    _predict_banner = ("Calculating predictive mean and variance...", " ")

    def _hist_width(self):
        return self._spec.n_params

    def _fit(self, T, hist, loss):
        return self._solver.fit(self, float(self.learning_rate), T, hist, loss)

    def _record(self, i, row, loss_i, show):
        n_ls = self._spec.n_ls
        if self._solver.xu_rows is not None:
            self.indpoints_all.append(self._solver.xu_rows[i])
        self.lscales.append(float(row[1]) if self._spec.isotropic else row[1:1 + n_ls].tolist())
        self.amp_all.append(float(row[0]))
        self.noise_all.append(float(row[1 + n_ls]))
        self.loss_all.append(float(loss_i))
        if show:
            return ('amp: {} ...'.format(np.around(self.amp_all[-1], 4)),
                    'length: {} ...'.format(np.around(self.lscales[-1], 4)),
                    'noise: {} ...'.format(np.around(self.noise_all[-1], 7)))

    def _print_final(self, T):
        var, ls, noise = self._spec.constrained(self._u)
        print('Final parameter values:\n',
              'amp: {}, lengthscale: {}, noise: {}'.format(
                  np.around(var.item(), 4), np.around(ls.tolist(), 4), np.around(noise.item(), 7)))

    # ------------------------------------------------------------------ prediction
    def _new_test_grid(self, Xtest):
        if Xtest is None:
            self._Xtest_d = self._Xd
        else:
            self._Xtest_d = self._to_device(self.Xtest)
            self.fulldims = Xtest.shape[1:]
            self._solver.new_test_grid(Xtest)

    def _posterior(self, predict, *Xs):
        """(mean, var) device tensors from ``predict`` of the solver: at the rows Xs[0], or on the stored test grid."""
        self._check_data()
        M = (Xs[0] if Xs else self._Xtest_d).shape[0]
        mean = torch.empty((M,), dtype=_F64, device=self._dev)
        var = torch.empty((M,), dtype=_F64, device=self._dev)
        _lib.check(predict(self, *Xs, mean, var))
        return mean, var

    def predict(self, Xtest=None, **kwargs):
        """Posterior mean and standard deviation (noise included) on the test grid;
        returns numpy arrays shaped like the grid (gpr.py:219-255)."""
        mean_h, sd_h, self._last_pred = self._predict_host(Xtest, kwargs, lambda: self._posterior(self._solver.predict_grid))
        return mean_h, sd_h

    def _predict_device(self, Xrows_d):
        """Posterior (mean, sd) device tensors at the (M, d) device rows `Xrows_d`; no host copies and no
        change of the stored test grid.  Internal: the device-resident acquisition path of boptimizer."""
        mean, var = self._posterior(self._solver.predict, Xrows_d)
        return mean, var.sqrt()

    # ------------------------------------------------------------------ joint posterior draws
    _SAMPLE_ENGINE = "joint posterior draws are built for the dense double-precision engine only (%s)"

    def _sample_supported(self):
        if self.do_sparse:
            raise NotImplementedError(self._SAMPLE_ENGINE % "sparse=True")
        if self.do_structured or self.do_symm:
            raise NotImplementedError(self._SAMPLE_ENGINE % "structured=True")
        if self.precision == "single":
            raise NotImplementedError(self._SAMPLE_ENGINE % "precision='single'")

    def _require_finite(self, Xrows_d):
        """ValueError unless the test rows are finite; one device-to-host look per tensor (boptimizer draws on the same
        grid at every step)."""
        if getattr(self, "_finite_rows", None) is Xrows_d:
            return
        if not bool(torch.isfinite(Xrows_d).all()):
            raise ValueError("sample: the test grid must be finite (NaN rows have no joint distribution)")
        self._finite_rows = Xrows_d

    def _sample_device(self, Xrows_d, z_d, noiseless=False, jitter=None):
        """(samples (S, M), mean (M), var (M)) device tensors of joint draws at the (M, d) device rows `Xrows_d` with the
        standard normals `z_d` (S, M): samples[s] = mean + chol(Sigma) z_d[s].  One library call; mean and var are the
        posterior of predict() (noise included)."""
        self._sample_supported()
        self._check_data()
        S, M = z_d.shape
        N = self._Xd.shape[0]
        if Xrows_d.shape[0] != M:
            raise ValueError("z must have shape (n_samples, %d); got %s" % (Xrows_d.shape[0], tuple(z_d.shape)))
        self._require_finite(Xrows_d)
        jitter = self._spec.jitter if jitter is None else float(jitter)
        # the one large allocation of the call: the padded (N + M)^2 joint covariance (kept by the handle, grow-only)
        order = -(-(N + M) // 128) * 128
        need = order * (order + (16 if order >= 1024 else 0)) * 8
        if need > getattr(self, "_sample_bytes", 0):
            free = torch.cuda.mem_get_info(self._dev)[0]
            if need > free:
                raise MemoryError("sample: the joint covariance of %d training and %d test points needs %.2f GiB of device "
                                  "memory, %.2f GiB are free" % (N, M, need / 2.0 ** 30, free / 2.0 ** 30))
        out = torch.empty((S, M), dtype=_F64, device=self._dev)
        mean = torch.empty((M,), dtype=_F64, device=self._dev)
        var = torch.empty((M,), dtype=_F64, device=self._dev)
        _lib.check(self._solver.sample(self, Xrows_d, z_d, noiseless, jitter, mean, var, out))
        self._sample_bytes = max(need, getattr(self, "_sample_bytes", 0))
        return out, mean, var

    def _pathwise_grid(self, Xrows_d, grid_shape):
        """(dict of gprutils.pathwise_grid, its idx on the device) for the grid rows `Xrows_d` and the current training
        rows; kept while both tensors stay the same objects."""
        c = getattr(self, "_pw_cache", None)
        if c is not None and c[0] is Xrows_d and c[1] is self._Xd and c[2] == tuple(grid_shape):
            return c[3], c[4]
        d = self._spec.dim
        if len(grid_shape) != d or int(np.prod(grid_shape)) != Xrows_d.shape[0]:
            raise NotImplementedError("pathwise draws need a product grid: %d test rows do not fill a grid of shape %s in "
                                      "%d dimensions" % (Xrows_d.shape[0], tuple(grid_shape), d))
        Xg = Xrows_d.cpu().numpy().T.reshape((d,) + tuple(grid_shape))
        P = gprutils.pathwise_grid(Xg, self._Xd.cpu().numpy())
        idx_d = torch.from_numpy(P["idx"]).to(self._dev)
        self._pw_cache = (Xrows_d, self._Xd, tuple(grid_shape), P, idx_d)
        return P, idx_d

    def _sample_pathwise_device(self, Xrows_d, grid_shape, z_d, noiseless=False, jitter=None):
        """(samples (S, M), mean (M)) device tensors of pathwise draws (Matheron's rule) on the
        complete product grid of shape `grid_shape` whose (M, d) device rows are `Xrows_d`, with the standard normals
        `z_d` (S, M + N) when noiseless, else (S, 2 M + N), split [z_p | z_e | z_n].  One library call: a prior draw through
        the grid's reflection blocks plus one mean-type update against the factor of the training covariance."""
        self._sample_supported()
        self._check_data()
        self._require_finite(Xrows_d)
        M, N = Xrows_d.shape[0], self._Xd.shape[0]
        W = M + N + (0 if noiseless else M)
        if z_d.dim() != 2 or z_d.shape[1] != W:
            raise ValueError("z must have shape (n_samples, %d) for method='pathwise' (M = %d grid points, N = %d "
                             "observations%s); got %s" % (W, M, N, "" if noiseless else ", noise on the grid", tuple(z_d.shape)))
        jitter = self._spec.jitter if jitter is None else float(jitter)
        s = float(self._spec.constrained(self._u)[2]) + self._spec.jitter
        if not (0.0 < jitter <= s):
            raise ValueError("pathwise draws need 0 < jitter <= noise + the model's jitter = %g; got %g" % (s, jitter))
        P, idx_d = self._pathwise_grid(Xrows_d, grid_shape)
        # the large allocations of the call: one (M / 2^r)^2 block of the prior and the N^2 training covariance
        nq = int(np.prod([(n + 1) // 2 if k in P["dims"] else n for k, n in enumerate(P["shape"])]))
        need = 0
        for order in (-(-nq // 128) * 128, -(-N // 128) * 128):
            need += order * (order + (16 if order >= 1024 else 0)) * 8
        if need > getattr(self, "_pathwise_bytes", 0):
            free = torch.cuda.mem_get_info(self._dev)[0]
            if need > free:
                raise MemoryError("sample: a prior block of %d points and the covariance of %d training points need %.2f GiB "
                                  "of device memory, %.2f GiB are free" % (nq, N, need / 2.0 ** 30, free / 2.0 ** 30))
        out = torch.empty((z_d.shape[0], M), dtype=_F64, device=self._dev)
        mean = torch.empty((M,), dtype=_F64, device=self._dev)
        _lib.check(self._solver.sample_pathwise(self, Xrows_d, P, idx_d, z_d, noiseless, jitter, mean, out))
        self._pathwise_bytes = max(need, getattr(self, "_pathwise_bytes", 0))
        return out, mean

    _BLOCKS_ENGINE = "method='blocks' draws on a fully observed grid in double precision (%s)"

    def _sample_blocks_host(self, n_samples, Xtest, noiseless, seed, z, jitter):
        """sample(method='blocks'): every argument is checked before anything is stored, so a refused call leaves the model
        and its stored test grid as they were."""
        if self.do_sparse:
            raise NotImplementedError(self._BLOCKS_ENGINE % "sparse=True")
        if self.precision == "single":
            raise NotImplementedError(self._BLOCKS_ENGINE % "precision='single'")
        if self.do_border:
            raise NotImplementedError(self._BLOCKS_ENGINE % "the image has missing points: method='blocks' needs a fully "
                                      "observed grid")
        self._check_data()
        if Xtest is not None:
            if not np.isfinite(np.asarray(Xtest, dtype=np.float64)).all():
                raise ValueError("sample: the test grid must be finite (NaN rows have no joint distribution)")
            Xs, shape = self._to_device(gprutils.prepare_test_data(Xtest, precision=self.precision)), tuple(Xtest.shape[1:])
        elif self._Xtest_d is not None:
            Xs, shape = self._Xtest_d, tuple(self.fulldims)
        else:
            Xs, shape = self._Xd, tuple(self.fulldims)
        self._require_finite(Xs)
        P, idx_d = self._pathwise_grid(Xs, shape)
        M, N = Xs.shape[0], self._Xd.shape[0]
        if N != M:          # (distinct rows, each on the grid: fewer of them than grid points)
            first = int(np.setdiff1d(np.arange(M), P["idx"])[0])
            raise NotImplementedError("method='blocks' needs an observation on every point of the test grid (the test grid "
                                      "must be the training grid): grid point %s has none (%d observations, %d grid points)"
                                      % (tuple(int(v) for v in np.unravel_index(first, shape)), N, M))
        W = 2 * M + (0 if noiseless else M)
        S = int(n_samples)
        if z is None:
            z_d = self._draw_z(S, W, seed)
        else:
            z_d = self._to_device(np.asarray(z) if not torch.is_tensor(z) else z)
            if z_d.dim() != 2 or z_d.shape != (S, W):
                raise ValueError("z must have shape (n_samples, %d) = (%d, %d) for method='blocks' (M = %d grid points%s); got %s"
                                 % (W, S, W, M, "" if noiseless else ", noise on the grid", tuple(z_d.shape)))
        jitter = self._spec.jitter if jitter is None else float(jitter)
        s = float(self._spec.constrained(self._u)[2]) + self._spec.jitter
        if not (0.0 < jitter <= s):
            raise ValueError("method='blocks' needs 0 < jitter <= noise + the model's jitter = %g; got %g" % (s, jitter))
        # the large allocation of the call: one (M / 2^r)^2 reflection block, reused by all 2 x 2^r factorisations
        nq = int(np.prod([(n + 1) // 2 if k in P["dims"] else n for k, n in enumerate(P["shape"])]))
        order = -(-nq // 128) * 128
        need = order * (order + (16 if order >= 1024 else 0)) * 8
        if need > getattr(self, "_blocks_bytes", 0):
            free = torch.cuda.mem_get_info(self._dev)[0]
            if need > free:
                raise MemoryError("sample: a reflection block of %d points needs %.2f GiB of device memory, %.2f GiB are free"
                                  % (nq, need / 2.0 ** 30, free / 2.0 ** 30))
        if Xtest is not None:
            self._resolve_test_grid(Xtest)
        out = torch.empty((S, M), dtype=_F64, device=self._dev)
        mean = torch.empty((M,), dtype=_F64, device=self._dev)
        Pd = dict(P, idx_d=None if np.array_equal(P["idx"], np.arange(M)) else idx_d)
        _lib.check(self._solver.sample_blocks(self, Xs, Pd, z_d, noiseless, jitter, mean, out))
        self._blocks_bytes = max(need, getattr(self, "_blocks_bytes", 0))
        return out.cpu().numpy().reshape((S,) + shape).astype(self._np_out, copy=False)

    _BORDER_ENGINE = "method='border' draws on an image with missing points through its bordered reflection blocks, in " \
                     "double precision (%s)"

    def _sample_border_host(self, n_samples, Xtest, noiseless, seed, z, jitter):
        """sample(method='border'): every argument is checked before anything is stored, so a refused call leaves the model
        and its stored test grid as they were."""
        if self.do_sparse:
            raise NotImplementedError(self._BORDER_ENGINE % "sparse=True")
        if self.precision == "single":
            raise NotImplementedError(self._BORDER_ENGINE % "precision='single'")
        if not self.do_border:
            if self.do_symm or self.do_structured:
                raise NotImplementedError(self._BORDER_ENGINE % "the grid is fully observed: use method='blocks'")
            raise NotImplementedError(self._BORDER_ENGINE % "a dense model: use method='pathwise', or skreconstructor for an "
                                      "image or cube with missing pixels")
        self._check_data()
        B = self._solver.S
        gshape = tuple(len(c) for c in B["axes"])
        if Xtest is not None:
            if not np.isfinite(np.asarray(Xtest, dtype=np.float64)).all():
                raise ValueError("sample: the test grid must be finite (NaN rows have no joint distribution)")
            Xs, shape = self._to_device(gprutils.prepare_test_data(Xtest, precision=self.precision)), tuple(Xtest.shape[1:])
        elif self._Xtest_d is not None:
            Xs, shape = self._Xtest_d, tuple(self.fulldims)
        else:
            Xs, shape = None, gshape
        c = getattr(self, "_border_grid", None)
        if c is None:
            G = np.array(np.meshgrid(*B["axes"], indexing="ij")).reshape(len(gshape), -1).T
            c = self._border_grid = [self._to_device(np.ascontiguousarray(G)),
                                     torch.from_numpy(B["miss"].astype(np.int64)).to(self._dev), None]
        G_d, miss_d = c[0], c[1]
        if Xs is not None and c[2] is not Xs:
            self._require_finite(Xs)
            if shape != gshape or Xs.shape != G_d.shape or not bool(torch.equal(Xs, G_d)):
                raise NotImplementedError("method='border' needs the completed training grid as its test grid (Xtest None, the "
                                          "stored grid, or a grid equal to it: shape %s); got a grid of shape %s that is not it"
                                          % (gshape, shape))
            if Xtest is None:
                c[2] = Xs                   # the stored grid: compared once
        M = G_d.shape[0]
        W = 2 * M + (0 if noiseless else M)
        S = int(n_samples)
        if z is None:
            z_d = self._draw_z(S, W, seed)
        else:
            z_d = self._to_device(np.asarray(z) if not torch.is_tensor(z) else z)
            if z_d.dim() != 2 or z_d.shape != (S, W):
                raise ValueError("z must have shape (n_samples, %d) = (%d, %d) for method='border' (M = %d grid points%s); got %s"
                                 % (W, S, W, M, "" if noiseless else ", noise on the grid", tuple(z_d.shape)))
        jitter = self._spec.jitter if jitter is None else float(jitter)
        s = float(self._spec.constrained(self._u)[2]) + self._spec.jitter
        if not (0.0 < jitter <= s):
            raise ValueError("method='border' needs 0 < jitter <= noise + the model's jitter = %g; got %g" % (s, jitter))
        # the large allocation beyond a prediction of the model: one (M / 2^r)^2 block for the prior factors
        nq = B["Xq"].shape[0]
        order = -(-nq // 128) * 128
        need = order * (order + (16 if order >= 1024 else 0)) * 8
        if need > getattr(self, "_border_bytes", 0):
            free, total = torch.cuda.mem_get_info(self._dev)
            if need > free:
                raise MemoryError("sample: a reflection block of %d points needs %.2f GiB of device memory, %.2f of %.2f GiB are "
                                  "free" % (nq, need / 2.0 ** 30, free / 2.0 ** 30, total / 2.0 ** 30))
        if Xtest is not None:
            self._resolve_test_grid(Xtest)
        out = torch.empty((S, M), dtype=_F64, device=self._dev)
        mean = torch.empty((M,), dtype=_F64, device=self._dev)
        P = {"shape": gshape, "mask": B["mask"], "twoc": B["twoc"]}
        _lib.check(self._solver.sample_border(self, G_d, P, miss_d, z_d, noiseless, jitter, mean, out))
        self._border_bytes = max(need, getattr(self, "_border_bytes", 0))
        return out.cpu().numpy().reshape((S,) + gshape).astype(self._np_out, copy=False)

    _KRON_ENGINE = "method='kron' draws through the Kronecker eigenbasis: reconstructor(..., kernel='RBF', structured=True) " \
                   "or skreconstructor(..., 'RBF') on a fully observed grid, in double precision (%s)"

    def _sample_kron_host(self, n_samples, Xtest, noiseless, seed, z, jitter):
        """sample(method='kron'): every argument is checked before anything is stored, so a refused call leaves the model,
        its stored test grid and the solver's test axes as they were."""
        sol = self._solver
        if not isinstance(sol, _solvers.Kron):
            what = ("sparse=True" if self.do_sparse else "the image has missing points: use method='border'" if self.do_border
                    else "a reflection-block model: use method='blocks'" if self.do_symm
                    else "a dense model: use method='joint' or 'pathwise'")
            raise NotImplementedError(self._KRON_ENGINE % what)
        if self.precision == "single":
            raise NotImplementedError(self._KRON_ENGINE % "precision='single'")
        self._check_data()
        if Xtest is not None:
            if not np.isfinite(np.asarray(Xtest, dtype=np.float64)).all():
                raise ValueError("sample: the test grid must be finite (NaN rows have no joint distribution)")
            try:
                taxes = gprutils.grid_axes(Xtest)[0]
            except NotImplementedError as e:
                raise NotImplementedError("method='kron' needs a product test grid: %s" % e)
            shape = tuple(np.shape(Xtest)[1:])
        else:
            taxes, shape = sol.taxes[0], tuple(self.fulldims)
            if not all(np.isfinite(t).all() for t in taxes):
                raise ValueError("sample: the test grid must be finite (NaN rows have no joint distribution)")
        union = gprutils.union_axes(sol.axes, taxes)
        for i, a in enumerate(union[0]):
            if len(a) > 4096:
                raise NotImplementedError("method='kron': the union of the training and the test coordinates of axis %d has "
                                          "%d entries, the eigen-solver takes at most 4096" % (i, len(a)))
        PU = int(np.prod([len(a) for a in union[0]], dtype=np.int64))
        N, M = self._Xd.shape[0], int(np.prod(shape, dtype=np.int64))
        W = PU + N + M
        S = int(n_samples)
        if S < 1:
            raise ValueError("n_samples must be at least 1; got %r" % (n_samples,))
        parts = "[zeta | z_e | z_n] = %d union-grid points + %d observations + %d test points" % (PU, N, M)
        if z is not None:
            zt = z if torch.is_tensor(z) else np.asarray(z)
            if zt.ndim != 2 or tuple(zt.shape) != (S, W):
                raise ValueError("z must have shape (n_samples, %d) = (%d, %d) for method='kron' (%s); got %s"
                                 % (W, S, W, parts, tuple(zt.shape)))
        jitter = self._spec.jitter if jitter is None else float(jitter)
        if not (0.0 <= jitter < np.inf):
            raise ValueError("method='kron' needs a finite jitter >= 0; got %g" % jitter)
        # what the call allocates: z, the draws and the mean here; in the library (csrc/kron.hip) zeta and the two buffers of
        # the mode products (S x the largest tensor a chain of mode products passes through), the gathered root rows, the
        # union axes' matrices when the training decomposition does not serve, and the prediction workspace
        nu, nn, nm = [len(a) for a in union[0]], [len(c) for c in sol.axes], [len(t) for t in taxes]
        smax, pmax = max(N, M), N
        for src, dst in ((nu, nn), (nu, nm), (nn, nm)):
            cur = int(np.prod(src, dtype=np.int64))
            for a, b in zip(src, dst):
                cur = cur // a * b
                smax = max(smax, cur)
                if src is nn:
                    pmax = max(pmax, cur)
        shared = nu == nn and all(np.array_equal(i, np.arange(len(i))) for i in union[1])
        lib_axes = 0 if shared else 2 * sum(nu) + 5 * sum(a * a for a in nu)
        lib_rows = sum((a + b) * c for a, b, c in zip(nn, nm, nu))
        lib_pred = sum(nm) + 2 * sum(a * b for a, b in zip(nn, nm)) + 2 * pmax
        z_on_device = torch.is_tensor(z) and z.is_cuda and z.dtype == _F64
        need = 8 * (S * ((0 if z_on_device else W) + M + PU + 2 * smax) + M + lib_axes + lib_rows + lib_pred)
        if need > getattr(self, "_kron_bytes", 0):
            free = torch.cuda.mem_get_info(self._dev)[0]
            if need > free:
                raise MemoryError("sample: %d draws on %d test points through %d union-grid points need %.2f GiB of device "
                                  "memory, %.2f GiB are free" % (S, M, PU, need / 2.0 ** 30, free / 2.0 ** 30))
        z_d = self._draw_z(S, W, seed) if z is None else self._to_device(z if torch.is_tensor(z) else np.asarray(z))
        if Xtest is not None:
            self._resolve_test_grid(Xtest)
        out = torch.empty((S, M), dtype=_F64, device=self._dev)
        mean = torch.empty((M,), dtype=_F64, device=self._dev)
        _lib.check(sol.sample_kron(self, taxes, union, z_d, noiseless, jitter, mean, out))
        self._kron_bytes = max(need, getattr(self, "_kron_bytes", 0))
        return out.cpu().numpy().reshape((S,) + shape).astype(self._np_out, copy=False)

    _COLUMNS_ENGINE = "method='columns' draws through the dense-by-Kronecker blocks: skreconstructor(..., 'RBF') whose solver " \
                      "is 'columns' (whole columns of the grid missing), in double precision (%s)"

    def _sample_columns_host(self, n_samples, Xtest, noiseless, seed, z, jitter):
        """sample(method='columns'): every argument is checked before anything is stored, so a refused call leaves the model,
        its stored test grid and the solver's test axes as they were."""
        sol = self._solver
        if not isinstance(sol, _solvers.Columns):
            what = ("sparse=True" if self.do_sparse else "the missing points are scattered: use method='border'" if self.do_border
                    else "the Kronecker model of a complete grid: use method='kron'" if isinstance(sol, _solvers.Kron)
                    else "a reflection-block model: use method='blocks'" if self.do_symm
                    else "a dense model: use method='joint' or 'pathwise'")
            raise NotImplementedError(self._COLUMNS_ENGINE % what)
        if self.precision == "single":
            raise NotImplementedError(self._COLUMNS_ENGINE % "precision='single'")
        self._check_data()
        if Xtest is not None:
            if not np.isfinite(np.asarray(Xtest, dtype=np.float64)).all():
                raise ValueError("sample: the test grid must be finite (NaN rows have no joint distribution)")
            try:
                taxes = gprutils.grid_axes(Xtest)[0]
            except NotImplementedError as e:
                raise NotImplementedError("method='columns' needs a product test grid: %s" % e)
            shape = tuple(np.shape(Xtest)[1:])
        else:
            taxes, shape = sol.taxes, tuple(self.fulldims)
            if taxes is None:
                raise NotImplementedError("method='columns' needs a product test grid: the model holds none (pass Xtest)")
            if not all(np.isfinite(t).all() for t in taxes):
                raise ValueError("sample: the test grid must be finite (NaN rows have no joint distribution)")
        S = int(n_samples)
        if S < 1:
            raise ValueError("n_samples must be at least 1; got %r" % (n_samples,))
        jitter = self._spec.jitter if jitter is None else float(jitter)
        if not (0.0 < jitter < np.inf):
            raise ValueError("method='columns' needs a finite jitter > 0 (the prior factor of the ragged rows); got %g" % jitter)
        geometry = sol.sample_geometry(taxes)
        rows, caxes, (P, _, _), (au, ic, _) = geometry
        for i, a in enumerate(au):
            if len(a) > 4096:
                raise NotImplementedError("method='columns': the union of the training and the test coordinates of axis %d has "
                                          "%d entries, the eigen-solver takes at most 4096" % (sol.C["complete"][i], len(a)))
        Us, U = len(P), int(np.prod([len(a) for a in au], dtype=np.int64))
        N, M = self._Xd.shape[0], int(np.prod(shape, dtype=np.int64))
        W = Us * U + N + M
        parts = "[zeta | z_e | z_n] = %d x %d union rows x union-axes points + %d observations + %d test points" % (Us, U, N, M)
        if z is not None:
            zt = z if torch.is_tensor(z) else np.asarray(z)
            if zt.ndim != 2 or tuple(zt.shape) != (S, W):
                raise ValueError("z must have shape (n_samples, %d) = (%d, %d) for method='columns' (%s); got %s"
                                 % (W, S, W, parts, tuple(zt.shape)))
        # what the call allocates: z (as given and in the library's layout), the draws twice and the mean here; in the library
        # (csrc/api.hip: gpimhip_sample_pkron) the prior factor, zeta and H, the mode products' and the blocks' buffers
        Ns, J = sol.C["Y"].shape
        need = 8 * (S * ((1 if torch.is_tensor(z) and z.is_cuda and z.dtype == _F64 else 2) * W + 2 * M) + 2 * M
                    + self._columns_library_doubles(S, Ns, len(rows), Us, J, [len(a) for a in au],
                                                    [len(c) for c in sol.C["axes_c"]], [len(c) for c in caxes]))
        if need > getattr(self, "_columns_bytes", 0):
            free = torch.cuda.mem_get_info(self._dev)[0]
            if need > free:
                raise MemoryError("sample: %d draws on %d test points through %d x %d union points need %.2f GiB of device "
                                  "memory, %.2f GiB are free" % (S, M, Us, U, need / 2.0 ** 30, free / 2.0 ** 30))
        z_d = self._draw_z(S, W, seed) if z is None else self._to_device(z if torch.is_tensor(z) else np.asarray(z))
        if Xtest is not None:
            self._resolve_test_grid(Xtest)
        out = torch.empty((S, M), dtype=_F64, device=self._dev)
        mean = torch.empty((M,), dtype=_F64, device=self._dev)
        _lib.check(sol.sample_columns(self, taxes, z_d, noiseless, jitter, mean, out, geometry))
        self._columns_bytes = max(need, getattr(self, "_columns_bytes", 0))
        return out.cpu().numpy().reshape((S,) + shape).astype(self._np_out, copy=False)

    @staticmethod
    def _columns_library_doubles(S, Ns, Ms, Us, J, nu, nn, nm):
        """The doubles gpimhip_sample_pkron's own buffers take (its arena and the prediction slab), by the library's formulas."""
        pad = lambda n: -(-int(n) // 128) * 128
        np_, npU = pad(Ns), pad(Us)
        nb = np_ // 128
        mc = min(pad(Ms), max(128, (1 << 26) // (J * nb) // 128 * 128))
        U = int(np.prod(nu, dtype=np.int64))
        pmax, cur, cx, ct, maxX, maxT = 1, J, U, U, U, U
        for a, b, c in zip(nu, nn, nm):
            cur, cx, ct = cur // b * c, cx // a * b, ct // a * c
            pmax, maxX, maxT = max(pmax, cur), max(maxX, cx), max(maxT, ct)
        big = max(Ns * maxX, Ms * maxT)
        per_draw = 2 * npU * U + 3 * big + 2 * pmax * mc + J * (3 * np_ + mc)
        sg = max(1, min(S, (1 << 25) // per_draw))
        groups = -(-S // sg)
        sg = -(-S // groups)
        cols, Sp, rowsP = pad(sg * U), pad(sg), pad(sg * J)
        arena = npU * (npU + 16) + 2 * npU * cols + 3 * sg * big + 2 * J * np_ * Sp + rowsP * (np_ + mc) + 2 * sg * pmax * mc
        slab = np_ * (mc + 16) + nb * mc + pad(J) * mc + 4 * pmax * mc
        return arena + slab

    def _draw_z(self, n_samples, M, seed=None, generator=None):
        if generator is None and seed is not None:
            generator = torch.Generator(self._dev).manual_seed(int(seed))
        return torch.randn((n_samples, M), dtype=_F64, device=self._dev, generator=generator)

    def sample(self, n_samples=1, Xtest=None, noiseless=False, seed=None, z=None, jitter=None, method='joint'):
        """Joint draws from the posterior on the test grid: ndarray of shape ``(n_samples, *fulldims)``, each slice one
        plausible reconstruction ``mean + chol(Sigma) z_s`` with ``Sigma`` the full posterior covariance of the grid plus
        ``((0 if noiseless else noise) + jitter) I``.  ``Xtest`` as in ``predict``; ``jitter`` defaults to the model's.
        ``z``: optional ``(n_samples, M)`` array or device tensor of standard normals, used as is (the result is then a
        pure function of the model).  When absent it is drawn as
        ``torch.randn((n_samples, M), dtype=torch.float64, device=dev, generator=g)`` with ``g = torch.Generator(dev).manual_seed(seed)``
        (``seed is None``: the global device generator).  Dense double-precision models only; the test grid must be
        finite.

        ``method='pathwise'`` (Matheron's rule) draws ``mean + g - (K_GX + d P)(K + s I)^-1 (g[idx] + sqrt(s - d) z_e)`` with
        ``g`` a prior draw on the grid: two factorisations of order M / 2^r and N instead of one of order N + M, for a test
        grid that is a complete product grid with a symmetric axis and holds every training row.  The same distribution up
        to terms of the size of ``jitter`` (0 < jitter <= noise + the model's jitter); ``z`` then has shape
        ``(n_samples, M + N)`` if noiseless, else ``(n_samples, 2 M + N)``, split ``[z_p | z_e | z_n]``, and is drawn by
        the rule above at that width.

        ``method='blocks'``: the pathwise draw for a model whose observations fill its grid -- ``reconstructor(...,
        structured=True)``, ``skreconstructor`` on a complete image or cube, or a dense double-precision model with an
        observation on every grid point -- computed in the grid's reflection basis alone: 2 x 2^r factorisations of order
        M / 2^r, no matrix of order M.  The test grid must be the training grid (``Xtest`` None, the
        stored grid, or equal to it) with a symmetric axis; ``z`` has shape ``(n_samples, 2 M)`` if noiseless, else
        ``(n_samples, 3 M)``, the layout of ``'pathwise'`` with N = M; 0 < jitter <= noise + the model's jitter.

        ``method='border'``: the pathwise draw for an image or cube with missing pixels -- ``skreconstructor`` whose
        ``solver`` is ``'border'`` -- through the bordered reflection blocks of the completed grid: the factorisations of a
        prediction plus 2^r prior factors of order M / 2^r, no matrix of the order of the image.  A
        draw fills the holes with one plausible reconstruction.  The test grid must be the completed training grid
        (``Xtest`` None, the stored grid, or equal to it); ``z`` has the layout of ``'blocks'``, every part indexed by the
        grid point (entries of ``z_e`` at missing pixels are ignored); 0 < jitter <= noise + the model's jitter.

        ``method='kron'``: Matheron's rule with every factor a Kronecker product, for the Kronecker model --
        ``reconstructor(..., kernel='RBF', structured=True)`` or ``skreconstructor(..., 'RBF')`` on a complete grid -- on ANY
        finite product test grid: the training grid, a finer one (``get_full_grid(dense_x=...)``), a shifted one, a crop
        (DESIGN.md section 21).  Nothing of the order of the image is factored: per axis one eigen-decomposition of the
        union of the training and the test coordinates (``gprutils.union_axes``), then mode products (measured: one draw
        costs 1.1 - 5 predictions, each of 16 draws 0.2 - 0.8).  The covariance of the draws is exactly the posterior's plus ``((0 if noiseless else noise) + jitter)
        I``, the distribution of ``'joint'``; ``jitter >= 0`` (0 allowed: no factorisation needs it).  ``z`` has shape
        ``(n_samples, prod U_i + N + M)`` whether noiseless or not, split ``[zeta | z_e | z_n]``: ``zeta`` row-major over
        the union axes (of orders ``U_i``), ``z_e`` in training-grid order, ``z_n`` in test-grid order.  A draw is a pure
        function of ``z`` on this engine; the prior root is fixed only up to an orthogonal change of ``zeta``, so draws
        for one ``z`` are not comparable with another implementation of the rule -- their distribution is.

        ``method='columns'``: Matheron's rule for a cube measured at a sparse set of pixels -- ``skreconstructor(..., 'RBF')``
        whose ``solver`` is ``'columns'`` -- on ANY finite product test grid.  A draw fills the
        unmeasured pixels with whole plausible spectra.  The prior goes through ``L_P = chol(s2 K_s(P, P) + jitter I)`` of
        the union ``P`` of the ragged (pixel) training and test rows (``gprutils.union_rows``, ``U_s`` rows) and the
        eigen-roots of the union of the complete (spectral) axes (``gprutils.union_axes``, orders ``U_i``), the update
        through the model's J blocks.  ``0 < jitter < inf`` (default: the model's).  The draws are exactly
        ``N(mean, Sigma_post + (0 if noiseless else noise) I + jitter T (I (x) K_c(u, u)) T^T)`` with
        ``T = S_* - K_*X (K_XX + (noise + model jitter) I)^-1 S_X`` (``S_X``, ``S_*`` select the training and the test points
        out of the union product grid, ``K_c(u, u)`` is the covariance of the union of the complete axes): the last term is
        positive semi-definite and of the size of ``jitter``, the price of factoring ``K_s(P, P)``, which is numerically
        singular on a pixel grid.  ``z`` has shape ``(n_samples, U_s prod U_i + N + M)`` whether noiseless or not, split
        ``[zeta | z_e | z_n]``: ``zeta`` row-major over ``(U_s, U_1, ...)``, ``z_e`` in the training points' row order,
        ``z_n`` in test-grid order.  ``z = 0`` gives ``predict``'s mean bit for bit.  The other five methods refuse this
        model, and ``'columns'`` refuses every other model, naming the method it has."""
        if method not in ("joint", "pathwise", "blocks", "border", "kron", "columns"):
            raise ValueError("method must be 'joint', 'pathwise', 'blocks', 'border', 'kron' or 'columns'; got %r" % (method,))
        if method == "columns":
            return self._sample_columns_host(n_samples, Xtest, noiseless, seed, z, jitter)
        if isinstance(self._solver, _solvers.Columns):
            raise NotImplementedError(self._solver._NO_DRAWS + " (got method=%r)" % (method,))
        if method == "kron":
            return self._sample_kron_host(n_samples, Xtest, noiseless, seed, z, jitter)
        if method == "blocks":
            return self._sample_blocks_host(n_samples, Xtest, noiseless, seed, z, jitter)
        if method == "border":
            return self._sample_border_host(n_samples, Xtest, noiseless, seed, z, jitter)
        self._sample_supported()
        if Xtest is not None and not np.isfinite(np.asarray(Xtest, dtype=np.float64)).all():
            # (refused before it replaces the stored test grid)
            raise ValueError("sample: the test grid must be finite (NaN rows have no joint distribution)")
        if method == "pathwise" and Xtest is not None:
            # a grid the method cannot take (not a product grid, no symmetric axis, a training row off it), like any other
            # refused argument, leaves the stored test grid as it was (the dense solver keeps no grid state of its own)
            kept = (self.Xtest, self._Xtest_d, self.fulldims)
            try:
                return self._sample_host(n_samples, Xtest, noiseless, seed, z, jitter, method)
            except Exception:
                self.Xtest, self._Xtest_d, self.fulldims = kept
                raise
        return self._sample_host(n_samples, Xtest, noiseless, seed, z, jitter, method)

    def _sample_host(self, n_samples, Xtest, noiseless, seed, z, jitter, method):
        self._resolve_test_grid(Xtest)
        Xs = self._Xtest_d
        M = Xs.shape[0]
        if method == "pathwise":
            M = M + self._Xd.shape[0] + (0 if noiseless else M)       # the width of z; the draws are (n_samples, grid)
        if z is None:
            z_d = self._draw_z(int(n_samples), M, seed)
        else:
            z_d = self._to_device(np.asarray(z) if not torch.is_tensor(z) else z)
            if z_d.dim() != 2 or z_d.shape != (int(n_samples), M):
                raise ValueError("z must have shape (n_samples, %d) = (%d, %d); got %s"
                                 % (M, int(n_samples), M, tuple(z_d.shape)))
        if method == "pathwise":
            out, _ = self._sample_pathwise_device(Xs, tuple(self.fulldims), z_d, noiseless, jitter)
        else:
            out, _, _ = self._sample_device(Xs, z_d, noiseless, jitter)
        return out.cpu().numpy().reshape((z_d.shape[0],) + tuple(self.fulldims)).astype(self._np_out, copy=False)

    def run(self, **kwargs):
        """train + predict; returns (mean, sd, hyperparams) (gpr.py:257-283)."""
        if kwargs.get("learning_rate") is not None:
            self.learning_rate = kwargs.get("learning_rate")
        if kwargs.get("iterations") is not None:
            self.iterations = kwargs.get("iterations")
        self.train(learning_rate=self.learning_rate, iterations=self.iterations)
        mean, sd = self.predict()
        return mean, sd, self.hyperparams

    def step(self, *args, **kwargs):
        """Dead code in the reference (gpr.py:285-329 calls ``gprutils.acquisition``, which does not
        exist, and fails with AttributeError); use ``boptimizer`` for exploration steps."""
        raise AttributeError("module 'gpim.gprutils' has no attribute 'acquisition' "
                             "(reconstructor.step is dead code in the reference; use boptimizer)")

    # ------------------------------------------------------------------ operator-level hooks
    def loss_and_grad(self):
        """(loss, d loss/du) at the current hyper-parameters; used by the parity tests."""
        self._check_data()
        out = torch.empty((1 + self._u.numel(),), dtype=_F64, device=self._dev)
        _lib.check(self._solver.nll_grad(self, out))
        o = out.cpu()
        return o[0].item(), o[1:].clone()
