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

from . import _lib, _sampling, _solvers, gprutils
from .kernels import get_kernel

_F64 = torch.float64


def _finite_test_grid(Xtest, who):
    """ValueError (its message opens with ``who``) for a test grid with NaN / inf entries; None is the stored grid."""
    if Xtest is not None and not np.isfinite(np.asarray(Xtest, dtype=np.float64)).all():
        raise ValueError("%s: the test grid must be finite (NaN / inf rows have no covariance with the others)" % who)


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
        self._o._data_swapped = True
        self._o._Xd = self._o._to_device(value)

    @property
    def y(self):
        return self._o._yd

    @y.setter
    def y(self, value):
        self._o._no_swap("y")
        self._o._data_swapped = True
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
        **objective (str): gpim_amd extension -- what ``train`` / ``run`` minimise and ``loss_and_grad`` evaluates: 'nll'
            (default), the negative log marginal likelihood, or 'loo', the leave-one-out pseudo-likelihood (Rasmussen &
            Williams 5.4.2) ``-sum_i log N(y_i | mu_-i, 1 / d_i)`` plus the same prior constant, with
            ``mu_-i`` the prediction of y_i from the other observations and ``d = diag(S^-1)``, S = K + (noise + jitter) I:
            the quantity ``loo()["elpd"]`` scores, as a training objective for a kernel that is only approximately right.
            The held-out variance is ``1 / d_i``, that of the matrix that is trained: ``loo()``'s reported variance plus
            the jitter wherever ``loo()`` did not clamp.  About twice the cost of an iteration on 'nll' (one more N^3
            product).  Dense double-precision models only: ``sparse=True``, ``structured=True`` and ``precision='single'``
            raise NotImplementedError with the reason; any other value raises ValueError.
    """

    def __init__(self, X, y, Xtest=None, kernel='RBF', lengthscale=None, sparse=False,
                 indpoints=None, learning_rate=5e-2, iterations=1000, use_gpu=False,
                 verbose=1, seed=0, **kwargs):
        self.precision = kwargs.get("precision", "double")
        self._np_out = np.float32 if self.precision == "single" else np.float64
        self.objective = _solvers.check_objective(kwargs.get("objective", "nll"))
        if self.objective == "loo":         # (before anything touches the device: the refusals need none)
            family = _solvers.Sparse if sparse else None
            if kwargs.get("structured", False):
                family = _solvers.Kron if kernel == "RBF" and kwargs.get("_border") is None and kwargs.get("_columns") is None \
                    else _solvers.Columns if kwargs.get("_columns") is not None else _solvers.Reflection
            _solvers.refuse_loo_objective("%s solver" % family.__name__ if family else "dense model",
                                          family.no_loo_objective if family else None, self.precision)
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
        # where the training rows sit in y as given (row-major): what loo(as_grid=True) scatters its results back to
        self._obs_mask = ~np.isnan(np.asarray(y, dtype=np.float64))
        self._data_swapped = False                      # model.X / model.y replaced: the rows no longer belong to that grid
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
        self._draw_bytes = {}        # method -> the largest sample() call that has run (_sampling.reserve)

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
        fit = self._solver.loo_fit if self.objective == "loo" else self._solver.fit
        return fit(self, float(self.learning_rate), T, hist, loss)

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

    def loo(self, as_grid=True):
        """Leave-one-out cross-validation at the current hyper-parameters, from ONE factorisation:
        ``(mean, sd, score)`` with ``mean[i]``, ``sd[i]`` the prediction of observation i from all the others (noise
        included, the convention of ``predict``) and ``score = {"elpd": sum_i log N(y_i | mean_i, sd_i^2), "rmse":
        sqrt(sum_i (y_i - mean_i)^2 / n), "n": n}`` -- a held-out measure that, unlike the training loss, is comparable
        across kernels and does not reward fitting the noise.  Costs less than one training iteration.

        ``as_grid=True``: arrays of the shape of ``y`` as given to the constructor, NaN where ``y`` was NaN (ValueError once
        the data were replaced through ``model.X`` / ``model.y``); ``as_grid=False``: flat arrays in the training rows'
        order.  dtype as ``predict``.  Dense models in either precision, and double-precision structured models on a complete grid (Kronecker, reflection
        blocks); sparse, border and column models raise NotImplementedError with the reason."""
        self._check_data()
        N = self._yd.shape[0]
        if as_grid and (self._data_swapped or int(self._obs_mask.sum()) != N):
            raise ValueError("loo(as_grid=True): the training data were replaced through model.X / model.y and no longer "
                             "belong to the grid of the constructor's y; use as_grid=False")
        mean = torch.empty((N,), dtype=_F64, device=self._dev)
        var = torch.empty((N,), dtype=_F64, device=self._dev)
        score = torch.empty((2,), dtype=_F64, device=self._dev)
        _lib.check(self._solver.loo(self, mean, var, score))
        elpd, sse = score.cpu().tolist()
        out = []
        for t in (mean, var.sqrt()):
            flat = t.cpu().numpy().astype(self._np_out, copy=False)
            if as_grid:
                full = np.full(self._obs_mask.shape, np.nan, dtype=self._np_out)
                full[self._obs_mask] = flat
                flat = full
            out.append(flat)
        return out[0], out[1], {"elpd": elpd, "rmse": float(np.sqrt(sse / N)), "n": N}

    def ivr(self, Xtest=None, weights=None, band=None):
        """Integrated variance reduction (ALC, the active-learning criterion of Cohn) on the test grid, at the current
        hyper-parameters: ``(ivr, mean, sd)``, numpy arrays of the grid's shape.  ``ivr[j] = sum_m w_m C_mj^2 / (C_jj +
        noise + jitter)`` with C the latent posterior covariance of the grid: the drop of the (weighted) total posterior
        variance of the whole grid when point j is measured -- the acquisition for the best reconstruction from the
        fewest measurements (the largest sd sits at the edges, where a measurement tells about the fewest other pixels).
        ``mean``, ``sd``: as ``predict``.  ``Xtest`` as in ``predict`` (finite); ``weights``: None or an array of the
        grid's shape, finite and >= 0 (ValueError otherwise).  Costs one product of M^2 N flop and M^2 doubles of device
        memory for M grid points.  ``band``: None keeps the covariance on the device; an int >= 1
        holds only that many of its 128-column block columns at a time -- M x (128 band + 16) doubles in place of M^2, the
        same product, the same map (section 30) -- and 'auto' chooses: None up to M = 16384, beyond it the widest band
        within 2 GiB (ValueError for anything else).  Dense double-precision models only: sparse, structured and
        single-precision models raise NotImplementedError with the reason."""
        from . import acqfunc
        _finite_test_grid(Xtest, "ivr")
        self._resolve_test_grid(Xtest)
        shape = tuple(self.fulldims)
        acq_d, mean_d, sd_d = acqfunc.ivr_on_device(self, self._Xtest_d, acqfunc._ivr_weights(weights, shape, self._dev),
                                                    band=band)
        self._last_pred = (mean_d, sd_d)
        host = torch.stack([acq_d, mean_d, sd_d]).cpu().numpy().astype(self._np_out, copy=False)
        return host[0].reshape(shape), host[1].reshape(shape), host[2].reshape(shape)

    def ivr_batch(self, n_points, Xtest=None, weights=None, mask=None, band=None):
        """A batch of ``n_points`` measurements chosen greedily by integrated variance reduction (``ivr``), at the current
        hyper-parameters: ``(points, gains, maps)``.  A GP's variance does not depend on the measured values, so the grid's
        covariance after measuring a point is known before the measurement; every pick is the maximiser of the ``ivr`` map
        conditioned on the picks before it, so two neighbouring maxima that explain the same pixels are not both taken.
        ``points``: list of grid-index tuples in pick order (fewer than ``n_points`` when the unmasked candidates run out);
        ``gains``: ndarray, the drop of the (weighted) total posterior variance each pick adds -- their sum is the batch's;
        ``maps``: dict with ``'ivr'`` (q, *grid), q = min(n_points, grid points): the map each pick was taken from (NaN at
        masked candidates and earlier picks, all NaN once the candidates have run out; ``maps['ivr'][0]`` is ``ivr()``'s
        map), ``'mean'``, ``'sd'``: as ``predict``, and ``'sd_after'``: the sd once the batch is measured.  ``Xtest``, ``weights`` as in ``ivr``; ``mask``: None or an array of the grid's shape
        holding 1 (a candidate) / NaN (excluded); it does not change the integral.  ValueError for n_points < 1, a grid that
        is not finite, bad weights or a bad mask.  One ``ivr`` plus one pass over the stored half of the covariance per
        further pick.  ``band`` as in ``ivr``: without the stored covariance every further pick
        costs a whole M^2 N product instead of one M^2 pass -- the price of the memory (section 30).  Dense
        double-precision models only, as ``ivr``."""
        from . import acqfunc
        if int(n_points) < 1:
            raise ValueError("ivr_batch: n_points must be >= 1; got %r" % (n_points,))
        _finite_test_grid(Xtest, "ivr")
        self._resolve_test_grid(Xtest)
        shape = tuple(self.fulldims)
        q = min(int(n_points), int(self._Xtest_d.shape[0]))
        return self._batch_result("ivr", q, shape, *acqfunc.ivr_greedy_on_device(
            self, self._Xtest_d, q, acqfunc._ivr_weights(weights, shape, self._dev), acqfunc._ivr_mask(mask, shape, self._dev),
            band=band))

    def _batch_result(self, key, q, shape, idx_d, val_d, count_d, maps_d, mean_d, sd_d, after_d):
        """``(points, values, maps)`` of ``ivr_batch`` (key 'ivr') / ``acq_batch`` (key 'acq') from the device tensors of
        their entry: the picks made, the maps in one stacked copy; (mean, sd) stay on the device as the last prediction."""
        self._last_pred = (mean_d, sd_d)
        n = int(count_d.item())
        flat = idx_d[:n].cpu().numpy()
        points = [tuple(int(v) for v in p) for p in np.stack(np.unravel_index(flat, shape), axis=-1)]
        host = torch.cat([maps_d, torch.stack([mean_d, sd_d, after_d])]).cpu().numpy().astype(self._np_out, copy=False)
        maps = {key: host[:q].reshape((q,) + shape), "mean": host[q].reshape(shape), "sd": host[q + 1].reshape(shape),
                "sd_after": host[q + 2].reshape(shape)}
        return points, val_d[:n].cpu().numpy().astype(self._np_out, copy=False), maps

    def acq_batch(self, n_points, acquisition_function='cb', Xtest=None, mask=None, alpha=0, beta=1, xi=0.01):
        """A batch of ``n_points`` measurements for the acquisition function 'cb', 'ei' or 'poi' by the kriging believer
        (GP-BUCB for 'cb'), at the current hyper-parameters: ``(points, values, maps)``.  After each pick the model is
        conditioned on the pick having been measured at its posterior mean -- the mean map stays, the variance drops as in
        ``ivr_batch`` -- and the next pick maximises the acquisition function of the conditioned model, so two neighbouring
        maxima that explain the same pixels are not both taken.  ``points``: list of grid-index tuples in pick order (fewer
        than ``n_points`` when the unmasked candidates run out); ``values``: ndarray, the map value each pick had when it
        was taken; ``maps``: dict with ``'acq'`` (q, *grid), q = min(n_points, grid points): the map each pick was taken
        from (NaN at masked candidates and earlier picks, all NaN once the candidates have run out), ``'mean'``, ``'sd'``:
        as ``predict``, and ``'sd_after'``: the sd once the batch is measured.  ``alpha``, ``beta``: of 'cb'; ``xi``: of
        'ei' / 'poi', whose incumbent is taken over the model's training inputs and the believed values.  ``Xtest``,
        ``mask`` as in ``ivr_batch``.  ValueError for n_points < 1, a grid that is not finite, a bad mask or another
        acquisition function.  One prediction plus one pass over L^-1 K(X, grid) per pick, no grid x grid matrix (DESIGN.md
        section 28).  Dense double-precision models only, as ``ivr``."""
        from . import acqfunc
        if acquisition_function not in ("cb", "ei", "poi"):
            raise ValueError("acq_batch: the acquisition function must be 'cb', 'ei' or 'poi'; got %r" % (acquisition_function,))
        if int(n_points) < 1:
            raise ValueError("acq_batch: n_points must be >= 1; got %r" % (n_points,))
        _finite_test_grid(Xtest, "acq_batch")
        self._solver._believer_supported(self)
        self._resolve_test_grid(Xtest)
        shape = tuple(self.fulldims)
        q = min(int(n_points), int(self._Xtest_d.shape[0]))
        return self._batch_result("acq", q, shape, *acqfunc.believer_on_device(
            self, acquisition_function, self._Xtest_d, q, p0=alpha, p1=beta, xi=xi,
            mask_d=acqfunc._ivr_mask(mask, shape, self._dev)))

    def _predict_device(self, Xrows_d):
        """Posterior (mean, sd) device tensors at the (M, d) device rows `Xrows_d`; no host copies and no
        change of the stored test grid.  Internal: the device-resident acquisition path of boptimizer."""
        mean, var = self._posterior(self._solver.predict, Xrows_d)
        return mean, var.sqrt()

    # ------------------------------------------------------------------ joint posterior draws (_sampling.py)
    def _sample_supported(self):
        _sampling.METHODS["joint"].gate(self)

    def _sample_device(self, Xrows_d, z_d, noiseless=False, jitter=None):
        """(samples (S, M), mean (M), var (M)) device tensors of joint draws at the (M, d) device rows `Xrows_d` with the
        standard normals `z_d` (S, M): samples[s] = mean + chol(Sigma) z_d[s].  One library call; mean and var are the
        posterior of predict() (noise included)."""
        return _sampling.draw_device(self, "joint", Xrows_d, None, z_d, noiseless, jitter)

    def _sample_pathwise_device(self, Xrows_d, grid_shape, z_d, noiseless=False, jitter=None):
        """(samples (S, M), mean (M)) device tensors of pathwise draws (Matheron's rule) on the
        complete product grid of shape `grid_shape` whose (M, d) device rows are `Xrows_d`, with the standard normals
        `z_d` (S, M + N) when noiseless, else (S, 2 M + N), split [z_p | z_e | z_n].  One library call: a prior draw through
        the grid's reflection blocks plus one mean-type update against the factor of the training covariance."""
        return _sampling.draw_device(self, "pathwise", Xrows_d, grid_shape, z_d, noiseless, jitter)[:2]

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
        if method not in _sampling.METHODS:
            raise ValueError("method must be 'joint', 'pathwise', 'blocks', 'border', 'kron' or 'columns'; got %r" % (method,))
        return _sampling.draw(self, method, n_samples, Xtest, noiseless, seed, z, jitter)

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
        """(loss, d loss/du) of the model's objective at the current hyper-parameters; used by the parity tests."""
        self._check_data()
        out = torch.empty((1 + self._u.numel(),), dtype=_F64, device=self._dev)
        _lib.check((self._solver.loo_grad if self.objective == "loo" else self._solver.nll_grad)(self, out))
        o = out.cpu()
        return o[0].item(), o[1:].clone()
