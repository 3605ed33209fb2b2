"""
_solvers.py -- the host layer between the reconstructors and the C ABI (include/gpimhip.h).

  * ``HostDriver``: the training driver and the predict prologue / epilogue shared by reconstructor, vreconstructor and
    smreconstructor; a class supplies its fit call, what it records per history row and its messages.
  * ``DeviceBlocks``: the device side of a blocks dict (gprutils.reflection_blocks* / border_blocks*), entered with
    ``_lib.reflection``.
  * ``Dense`` / ``Sparse`` / ``Kron`` / ``Columns`` / ``Reflection``: the engine paths of ``reconstructor``, one interface --
    fit(o, lr, T, hist, loss), predict(o, Xs, mean, var), predict_grid(o, mean, var), nll_grad(o, out),
    loo(o, mean, var, score), loo_fit / loo_grad (fit / nll_grad for ``objective='loo'``), each returning the library's status (a path without an exact leave-one-out raises
    NotImplementedError with its reason).  ``SpectralBlocks``: the reflection / border path of ``smreconstructor`` (one shared parameter vector).
    ``o`` is the owning reconstructor, passed per call: a solver never stores it (no reference cycle
    through the library handle) and reads ``o._Xd`` / ``o._yd`` / ``o._u`` as they are at the time of the call
    (boptimizer swaps the training data between trainings).  A new path is one more class here and one more arm where
    ``reconstructor.__init__`` builds ``self._solver``.
"""
import contextlib
import ctypes
import time
import warnings

import numpy as np
import torch

from . import _lib, gprutils
from ._lib import ptr

_F64 = torch.float64


class HostDriver:
    """``train`` and the host side of ``predict``.  The class provides: ``_hist_width()``, ``_fit(T, hist, loss) -> rc``,
    ``_record(i, row, loss_i, show)`` (appends to the histories; when ``show``, returns what the iteration line prints after
    the loss), ``_print_final(T)``, ``_new_test_grid(Xtest)`` (sets ``fulldims``; Xtest None: the training points) and the class constants."""
    _print_every, _avg_time_above = 10, 10      # verbose == 2 prints every n-th row; the average time is printed for T > n
    _predict_banner = ('Calculating predictive mean and uncertainty...', '\n')
    _np_out = np.float64

    def _check_data(self):
        pass

    def train(self, **kwargs):
        """Adam on the model's objective (the negative log marginal likelihood; ``reconstructor(objective='loo')``: the
        leave-one-out pseudo-likelihood); every call starts a fresh optimiser while the hyper-parameters
        persist (warm start), like the reference's train()."""
        for k in ("learning_rate", "iterations", "verbose"):
            if kwargs.get(k) is not None:
                setattr(self, k, kwargs.get(k))
        self._check_data()
        T = int(self.iterations)
        start_time = time.time()
        if self.verbose:
            print('Model training...')
        hist = torch.empty((max(T, 1), self._hist_width()), dtype=_F64, device=self._dev)
        loss = torch.empty((max(T, 1),), dtype=_F64, device=self._dev)
        rc = self._fit(T, hist, loss)
        failed = rc == _lib.E_NOT_PD
        if failed:
            # the device loop froze the parameters at the failing iteration: keep the history up to it
            # and raise what torch.linalg.cholesky raises there in the reference (gpr.py:192)
            T = int(self._handle.lib.gpimhip_fit_completed(self._handle.h))
        else:
            _lib.check(rc)
        hist_h, loss_h = hist[:T].cpu().numpy(), loss[:T].cpu().numpy()
        dt = time.time() - start_time
        for i in range(T):
            show = self.verbose == 2 and (i % self._print_every == 0 or i == T - 1)
            tail = self._record(i, hist_h[i], loss_h[i], show)
            if show:
                print('iter: {} ...'.format(i), 'loss: {} ...'.format(np.around(loss_h[i], 4)), *tail)
        if failed:
            _lib.check(rc)
        if self.verbose:
            if T > self._avg_time_above:
                print('average time per iteration: {} s'.format(np.round(dt / T, 6)))
            print('training completed in {} s'.format(np.round(dt, 2)))
            self._print_final(T)

    def run(self):
        """train() then predict(); returns mean, sd, hyperparams like the reference's run()."""
        self.train()
        mean, sd = self.predict()
        return mean, sd, self.hyperparams

    def _resolve_test_grid(self, Xtest):
        """The test grid of predict() / sample(): a new one when given, else the stored one, else the training points."""
        if Xtest is None and self.Xtest is None:
            warnings.warn("No test data provided. Using training data for prediction", UserWarning)
            self.Xtest = self.X
            self._new_test_grid(None)
        elif Xtest is not None:
            self.Xtest = gprutils.prepare_test_data(Xtest, precision=self.precision)
            self._new_test_grid(Xtest)

    def _predict_host(self, Xtest, kwargs, posterior):
        """Resolves the test grid, calls ``posterior() -> (mean, var)`` device tensors, and returns (mean, sd) as numpy arrays
        of shape ``fulldims`` plus the device pair (mean, sd)."""
        self._resolve_test_grid(Xtest)
        if kwargs.get("verbose") is not None:
            self.verbose = kwargs.get("verbose")
        if self.verbose:
            print(self._predict_banner[0], end=self._predict_banner[1])
        mean, var = posterior()
        sd = var.sqrt()
        mean_h = mean.cpu().numpy().reshape(self.fulldims).astype(self._np_out, copy=False)
        sd_h = sd.cpu().numpy().reshape(self.fulldims).astype(self._np_out, copy=False)
        if self.verbose:
            print("Done")
        return mean_h, sd_h, (mean, sd)


class DeviceBlocks:
    """A blocks dict S on the device: Xq, ys, wts (tiled once per task for a multi-output model) and the constants that
    ``_lib.reflection`` passes on; ``upload_border`` adds the missing points' representatives and coefficients."""

    def __init__(self, S, dev, tasks=None):
        self.S, self.dev = S, dev
        self.mask, self.n_total, self.B = S["mask"], S["n_total"], S["B"]
        self.twoc = (ctypes.c_double * 4)(*S["twoc"])
        self.Xq, self.ys = self._up(S["Xq"]), self._up(S["ys"])
        wts = S["wts"] if tasks is None or S["wts"] is None else np.tile(S["wts"], (tasks, 1))
        self.wts = None if wts is None else self._up(wts)
        self.border = None
        self.ones = None                                # (B, Nq) basis change of the constant mean, uploaded by SpectralBlocks

    def _up(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev, _F64).contiguous()

    def upload_border(self):
        self.q = torch.from_numpy(np.ascontiguousarray(self.S["q"], dtype=np.int32)).to(self.dev)
        self.coef = self._up(self.S["coef"])
        self.border = (len(self.S["miss"]), self.q, self.coef)


OBJECTIVES = ("nll", "loo")


def check_objective(objective):
    """'nll' (the negative log marginal likelihood) or 'loo' (the leave-one-out pseudo-likelihood); ValueError otherwise."""
    if objective not in OBJECTIVES:
        raise ValueError("objective must be 'nll' or 'loo'; got %r" % (objective,))
    return objective


def refuse_loo_objective(who, why=None, precision="double"):
    """NotImplementedError with the reason where objective='loo' cannot be trained: ``why`` (a model family's), or single
    precision."""
    if why is None and precision == "single":
        why = ("single precision does not resolve d = diag(S^-1) and the loss's log d (float matrices lose eps32 x the "
               "condition number): build the model with precision='double'")
    if why:
        raise NotImplementedError("objective='loo': the %s cannot train on the leave-one-out objective -- %s" % (who, why))


def _head(o):
    return o._handle.h, ctypes.byref(o._mstruct)


def _loss_grad(out):
    return ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(out.data_ptr() + 8)


class Dense:
    """The exact GP on the observed points (csrc/engine.hip, grad.hip, predict.hip)."""
    sparse = structured = symm = border = False         # what reconstructor shows as do_sparse / do_structured / ...
    xu_rows = None                                      # host rows of the inducing-input history of the latest fit (Sparse)

    def attach(self, o):
        """The device tensors a path uploads when the reconstructor is built (after its training and test data)."""

    def new_test_grid(self, Xtest):
        """predict() was given a new test grid."""

    def fit(self, o, lr, T, hist, loss):
        return o._handle.lib.gpimhip_fit_exact(*_head(o), ptr(o._Xd), ptr(o._yd), o._Xd.shape[0], ptr(o._u), lr, T,
                                               ptr(hist), ptr(loss))

    def predict(self, o, Xs, mean, var):
        return o._handle.lib.gpimhip_predict_exact(*_head(o), ptr(o._Xd), ptr(o._yd), o._Xd.shape[0], ptr(o._u), ptr(Xs),
                                                   Xs.shape[0], ptr(mean), ptr(var))

    def predict_grid(self, o, mean, var):
        return self.predict(o, o._Xtest_d, mean, var)

    def nll_grad(self, o, out):
        return o._handle.lib.gpimhip_nll_grad(*_head(o), ptr(o._Xd), ptr(o._yd), o._Xd.shape[0], ptr(o._u), *_loss_grad(out))

    # why a path cannot train on the leave-one-out objective (the paths that inherit Dense's methods below)
    no_loo_objective = None

    def _loo_objective_supported(self, o):
        refuse_loo_objective(type(self).__name__ + " solver", self.no_loo_objective, o.precision)

    def loo_fit(self, o, lr, T, hist, loss):
        """``fit`` on the leave-one-out pseudo-likelihood (csrc/loograd.hip): the dense
        double-precision model only."""
        self._loo_objective_supported(o)
        return o._handle.lib.gpimhip_fit_exact_loo(*_head(o), ptr(o._Xd), ptr(o._yd), o._Xd.shape[0], ptr(o._u), lr, T,
                                                   ptr(hist), ptr(loss))

    def loo_grad(self, o, out):
        """``nll_grad`` for the leave-one-out pseudo-likelihood."""
        self._loo_objective_supported(o)
        return o._handle.lib.gpimhip_loo_grad(*_head(o), ptr(o._Xd), ptr(o._yd), o._Xd.shape[0], ptr(o._u), *_loss_grad(out))

    no_loo = None                                       # why a path has no exact leave-one-out (the paths that inherit Dense's)

    def _loo_refused(self, why=None):
        raise NotImplementedError("loo(): the %s solver has no exact leave-one-out -- %s" % (type(self).__name__, why or self.no_loo))

    def loo(self, o, mean, var, score):
        """Leave-one-out predictions of the N training rows, in their order, and score = [elpd, sse] from one factorisation
        (csrc/predict.hip: colsq_tri_kernel, loo_finish_kernel).  Double- and single-precision models."""
        if self.no_loo:
            self._loo_refused()
        return o._handle.lib.gpimhip_loo_exact(*_head(o), ptr(o._Xd), ptr(o._yd), o._Xd.shape[0], ptr(o._u), ptr(mean), ptr(var),
                                               ptr(score))

    def _loo_double_only(self, o):
        if o.precision == "single":
            self._loo_refused("the structured solvers compute in double from float32 inputs, a mix that leave-one-out has no "
                              "stated accuracy for: build the model with precision='double'")

    no_ivr = None                                       # why a path has no integrated variance reduction

    def ivr(self, o, Xs, weights, mask, mean, sd, acq, band=None):
        """Integrated variance reduction at the rows Xs: acq[j] = sum_m w_m C_mj^2 / (max(C_jj, 0) + noise + jitter) with C the
        latent posterior covariance of the rows, and their posterior (mean, sd) (csrc/ivr.hip).
        weights, mask: device tensors of Xs.shape[0] doubles or None.  band: None (C is stored) or the block columns of C
        held at a time (gpimhip_ivr_exact_banded; section 30).  Dense double-precision models only."""
        self._ivr_supported(o)
        head = (*_head(o), ptr(o._Xd), ptr(o._yd), o._Xd.shape[0], ptr(o._u), ptr(Xs), Xs.shape[0])
        tail = (ptr(weights), ptr(mask), ptr(mean), ptr(sd), ptr(acq))
        if band is None:
            return o._handle.lib.gpimhip_ivr_exact(*head, *tail)
        return o._handle.lib.gpimhip_ivr_exact_banded(*head, int(band), *tail)

    def _needs_w(self, o, who, what, cancels):
        """Refuses what is built on W = L^-1 K(X, grid) (integrated variance reduction, believer batches) where the path has
        no such W (``no_ivr`` says why) or computes in single precision (``cancels``: what would cancel there)."""
        if self.no_ivr:
            raise NotImplementedError("%s: the %s solver has no %s -- %s" % (who, type(self).__name__, what, self.no_ivr))
        if o.precision == "single":
            raise NotImplementedError("%s: %s to the posterior variance, which single precision does not resolve: build the "
                                      "model with precision='double'" % (who, cancels))

    def _ivr_supported(self, o):
        self._needs_w(o, "ivr()", "integrated variance reduction", "C = K** - W^T W cancels")

    def ivr_greedy(self, o, Xs, weights, mask, q, mean, sd, maps, sd_after, idx, gain, count, band=None):
        """A greedy batch of q picks by integrated variance reduction at the rows Xs: pick r maximises the map of the
        covariance conditioned on picks 0 .. r - 1 (csrc/ivr.hip: gpimhip_ivr_greedy).  maps (q, M),
        sd_after (M), idx, gain (q), count (1): device tensors; the rest as ``ivr`` (band: gpimhip_ivr_greedy_banded, where a
        further pick costs a whole M^2 N product).  Dense double-precision models only."""
        self._ivr_supported(o)
        head = (*_head(o), ptr(o._Xd), ptr(o._yd), o._Xd.shape[0], ptr(o._u), ptr(Xs), Xs.shape[0])
        tail = (ptr(weights), ptr(mask), int(q), ptr(mean), ptr(sd), ptr(maps), ptr(sd_after), ptr(idx), ptr(gain), ptr(count))
        if band is None:
            return o._handle.lib.gpimhip_ivr_greedy(*head, *tail)
        return o._handle.lib.gpimhip_ivr_greedy_banded(*head, int(band), *tail)

    def believer(self, o, kind, Xs, Xobs, p0, p1, mask, q, mean, sd, maps, sd_after, idx, val, count):
        """A believer batch of q picks for the acquisition function kind ('cb' / 'ei' / 'poi') at the rows Xs: pick r
        maximises the acquisition function of the model conditioned on picks 0 .. r - 1 having been measured at their
        posterior means (csrc/believer.hip: gpimhip_acquire_batch).  Xobs: the observed rows (EI /
        POI) or None; (p0, p1) = (alpha, beta) for CB, (ignored, xi) else; the rest as ``ivr_greedy``.  Dense
        double-precision models only."""
        self._believer_supported(o)
        return o._handle.lib.gpimhip_acquire_batch(*_head(o), ptr(o._Xd), ptr(o._yd), o._Xd.shape[0], ptr(o._u), ptr(Xs),
                                                   Xs.shape[0], ptr(Xobs), 0 if Xobs is None else Xobs.shape[0], _lib.ACQ_IDS[kind],
                                                   float(p0), float(p1), ptr(mask), int(q), ptr(mean), ptr(sd), ptr(maps),
                                                   ptr(sd_after), ptr(idx), ptr(val), ptr(count))

    def _believer_supported(self, o):
        # (the paths without integrated variance reduction have no conditioned columns either, for the same reasons)
        self._needs_w(o, "acq_batch()", "believer batch", "v = s2 - sum W^2 and the conditioned columns cancel")

    def sample(self, o, Xs, z, noiseless, jitter, mean, var, out):
        """Joint posterior draws out[s] = mean + chol(Sigma) z[s] at the rows Xs (csrc/sample.hip).  The dense model only:
        the gate of _sampling.Joint refuses the other paths before a solver is asked."""
        return o._handle.lib.gpimhip_sample_exact(*_head(o), ptr(o._Xd), ptr(o._yd), o._Xd.shape[0], ptr(o._u), ptr(Xs),
                                                  Xs.shape[0], ptr(z), z.shape[0], int(bool(noiseless)), float(jitter),
                                                  ptr(mean), ptr(var), ptr(out))

    def sample_pathwise(self, o, Xs, P, idx, z, noiseless, jitter, mean, out):
        """Pathwise posterior draws on the complete grid whose rows are Xs (csrc/sample.hip):
        out[s] = mean + g_s - (K_GX + d P)(K + s I)^-1 (g_s[idx] + sqrt(s - d) z_e), g_s a prior draw through the grid's
        reflection blocks.  P: the dict of gprutils.pathwise_grid, idx: its flat training indices on the device, z:
        (S, M + N [+ M]).  The dense model only, as ``sample``."""
        d = o._spec.dim
        shape = (ctypes.c_int32 * d)(*[int(n) for n in P["shape"]])
        twoc = (ctypes.c_double * 4)(*P["twoc"])
        return o._handle.lib.gpimhip_sample_pathwise(*_head(o), ptr(Xs), shape, int(P["mask"]), twoc,
                                                     ctypes.c_void_p(idx.data_ptr()), ptr(o._yd), o._Xd.shape[0], ptr(o._u),
                                                     ptr(z), z.shape[0], int(bool(noiseless)), float(jitter), ptr(mean),
                                                     ptr(out))

    def sample_blocks(self, o, Xs, P, z, noiseless, jitter, mean, out):
        """Pathwise draws for observations on every point of the complete grid whose rows are Xs, block by block in the
        grid's reflection basis (csrc/sample.hip).  P: the dict of gprutils.pathwise_grid plus idx_d,
        the flat grid index of every training row on the device (None: the rows are in grid order); z: (S, 2 M [+ M]).
        The entry needs the grid, y and u only, so ``Kron`` and ``Reflection`` models on a complete grid inherit it."""
        d = o._spec.dim
        shape = (ctypes.c_int32 * d)(*[int(n) for n in P["shape"]])
        twoc = (ctypes.c_double * 4)(*P["twoc"])
        y = o._yd
        if P["idx_d"] is not None:
            y = torch.empty_like(o._yd)
            y[P["idx_d"]] = o._yd
        return o._handle.lib.gpimhip_sample_blocks(*_head(o), ptr(Xs), shape, int(P["mask"]), twoc, ptr(y), ptr(o._u), ptr(z),
                                                   z.shape[0], int(bool(noiseless)), float(jitter), ptr(mean), ptr(out))

    def sample_border(self, o, *args):
        """Draws through the bordered reflection blocks belong to the border solver (``Reflection(border=True)``)."""
        raise NotImplementedError("method='border' draws through the bordered reflection blocks of an image with missing "
                                  "points (the %s solver has none)" % type(self).__name__)

    def sample_kron(self, o, *args):
        """Draws through the Kronecker factors belong to the Kronecker model (``Kron``)."""
        raise NotImplementedError("method='kron' draws through the Kronecker eigenbasis of the structured RBF model on a "
                                  "complete grid (the %s solver has none)" % type(self).__name__)

    def sample_columns(self, o, *args):
        """Draws through the dense-by-Kronecker blocks belong to the column-blocks model (``Columns``)."""
        raise NotImplementedError("method='columns' draws through the dense-by-Kronecker blocks of a grid whose missing points "
                                  "are whole columns, solver='columns' (the %s solver has none)" % type(self).__name__)


class Sparse(Dense):
    """Sparse variational GP (VFE) with the ``o._n_ind`` trainable inducing inputs at the end of ``o._u`` (csrc/vfe.hip)."""
    sparse = True
    no_loo = ("the variational (VFE) posterior conditions on inducing points, not on the observations: dropping one "
              "observation has no closed form in its factors")
    no_ivr = "the posterior conditions on inducing points"
    no_loo_objective = ("sparse=True: the variational (VFE) bound conditions on inducing points, not on the observations, and "
                        "has no held-out terms to sum")

    def fit(self, o, lr, T, hist, loss):
        hist_xu = torch.empty((max(T, 1), o._n_ind, o._spec.dim), dtype=_F64, device=o._dev)
        rc = o._handle.lib.gpimhip_fit_vfe(*_head(o), ptr(o._Xd), ptr(o._yd), o._Xd.shape[0], o._n_ind, ptr(o._u), lr, T,
                                           ptr(hist), ptr(hist_xu), ptr(loss))
        self.xu_rows = hist_xu.cpu().numpy()
        return rc

    def predict(self, o, Xs, mean, var):
        return o._handle.lib.gpimhip_predict_vfe(*_head(o), ptr(o._Xd), ptr(o._yd), o._Xd.shape[0], o._n_ind, ptr(o._u),
                                                 ptr(Xs), Xs.shape[0], ptr(mean), ptr(var))

    def nll_grad(self, o, out):
        return o._handle.lib.gpimhip_vfe_nll_grad(*_head(o), ptr(o._Xd), ptr(o._yd), o._Xd.shape[0], o._n_ind, ptr(o._u),
                                                  *_loss_grad(out))


class Kron(Dense):
    """Exact GP through the Kronecker structure of the RBF covariance on a complete product grid (csrc/kron.hip)."""
    structured = True
    no_ivr = "the cross-covariance of arbitrary grid points is not block-structured"
    no_loo_objective = ("structured=True (Kronecker): the gradient needs S^-1 diag(omega) S^-1 contracted with dS, which does "
                        "not factorise over the axes' eigenbases; only the score rec.loo() does")

    def __init__(self, axes, axes_n):
        self.axes, self.axes_n = axes, axes_n
        self.taxes = (axes, axes_n)                     # the test grid's axes: the training grid until told otherwise

    def attach(self, o):
        self.axes_d = o._to_device(np.concatenate(self.axes))

    def new_test_grid(self, Xtest):
        self.taxes = gprutils.grid_axes(Xtest)

    def _grid(self, o):
        return (*_head(o), o._spec.dim, self.axes_n, ptr(self.axes_d), ptr(o._yd), ptr(o._u))

    def fit(self, o, lr, T, hist, loss):
        return o._handle.lib.gpimhip_fit_kron(*self._grid(o), lr, T, ptr(hist), ptr(loss))

    def predict(self, o, Xs, mean, var):
        raise NotImplementedError("structured models predict on product grids (use predict())")

    def predict_grid(self, o, mean, var):
        taxes, tn = self.taxes
        if int(np.prod([len(c) for c in taxes])) != mean.shape[0]:
            raise NotImplementedError("structured=True predicts on product grids only")
        return o._handle.lib.gpimhip_predict_kron(*self._grid(o), tn, ptr(o._to_device(np.concatenate(taxes))), ptr(mean),
                                                  ptr(var))

    def nll_grad(self, o, out):
        return o._handle.lib.gpimhip_kron_nll_grad(*self._grid(o), *_loss_grad(out))

    def loo(self, o, mean, var, score):
        """In the eigenbasis: diag(S^-1) = ((x) Q_i o Q_i)(1 / D) by mode products (csrc/kron.hip: gpimhip_loo_kron)."""
        self._loo_double_only(o)
        return o._handle.lib.gpimhip_loo_kron(*self._grid(o), ptr(mean), ptr(var), ptr(score))

    def sample_kron(self, o, taxes, union, z, noiseless, jitter, mean, out):
        """Joint posterior draws on the product grid of the axes ``taxes`` by Matheron's rule in Kronecker form (csrc/kron.hip:
        gpimhip_sample_kron).  union: what gprutils.union_axes returns for the training and the test
        axes; z: (S, prod U_i + N + M) device tensor [zeta | z_e | z_n]; mean (M), out (S, M)."""
        au, ic, it = union
        i32 = lambda v: (ctypes.c_int32 * len(v))(*[int(k) for k in v])
        # (both device tensors stay referenced until the call returns: a temporary's block would be handed to the next one)
        taxes_d, au_d = o._to_device(np.concatenate(taxes)), o._to_device(np.concatenate(au))
        return o._handle.lib.gpimhip_sample_kron(*self._grid(o), i32([len(t) for t in taxes]),
                                                 ptr(taxes_d), i32([len(a) for a in au]),
                                                 ptr(au_d), i32(np.concatenate(ic)),
                                                 i32(np.concatenate(it)), ptr(z), z.shape[0], int(bool(noiseless)),
                                                 float(jitter), ptr(mean), ptr(out))


class Columns(Dense):
    """Exact RBF GP on a grid whose missing points are whole columns (a cube measured at a sparse set of pixels, an image
    with whole rows missing): J dense blocks of the N_s observed ragged points, one per eigen-direction of the complete axes,
    in one lock-step batch (gprutils.column_blocks; csrc/pkron.hip).  ``o._u``, the loss, the history
    and the posterior are those of ``Dense`` on the same observations."""
    structured = True
    _NO_DRAWS = "solver='columns' draws with method='columns' only"
    no_ivr = "the cross-covariance of arbitrary grid points is not block-structured"
    no_loo_objective = ("solver='columns': diag(S^-1) of the dense-by-Kronecker blocks mixes every block's diagonal through "
                        "the complete axes' eigenvectors, which is not built")
    no_loo = ("solver='columns': diag(S^-1) of the dense-by-Kronecker blocks mixes every block's diagonal through the "
              "complete axes' eigenvectors, which is not built")

    def __init__(self, C):
        self.C = C
        self.taxes = None                               # the test grid's d coordinate vectors; None: the training points

    def attach(self, o):
        C = self.C
        i32 = lambda v: (ctypes.c_int32 * len(v))(*[int(k) for k in v])
        self.Xs_d, self.Y_d = o._to_device(C["Xs"]), o._to_device(C["Y"])
        self.axes_d = o._to_device(np.concatenate(C["axes_c"]))
        self.n_c, self.perm = i32([len(c) for c in C["axes_c"]]), i32(C["perm"])
        self._train_order = None

    def new_test_grid(self, Xtest):
        self.taxes = gprutils.grid_axes(Xtest)[0]

    def _model(self, o):
        C = self.C
        return (*_head(o), ptr(self.Xs_d), self.Xs_d.shape[0], len(C["ragged"]), len(C["complete"]), self.n_c, self.perm,
                ptr(self.axes_d), ptr(self.Y_d))

    def fit(self, o, lr, T, hist, loss):
        return o._handle.lib.gpimhip_fit_pkron(*self._model(o), ptr(o._u), lr, T, ptr(hist), ptr(loss))

    def nll_grad(self, o, out):
        return o._handle.lib.gpimhip_pkron_nll_grad(*self._model(o), ptr(o._u), *_loss_grad(out))

    def _predict_product(self, o, rows_d, caxes, mean, var):
        """The posterior on (the ragged rows rows_d (M_s, p)) x (the product of the complete axes' vectors caxes), M_s x M_c."""
        i32 = lambda v: (ctypes.c_int32 * len(v))(*[int(k) for k in v])
        caxes_d = o._to_device(np.concatenate(caxes))       # (referenced until the call returns)
        return o._handle.lib.gpimhip_predict_pkron(*self._model(o), ptr(o._u), ptr(rows_d), rows_d.shape[0],
                                                   i32([len(c) for c in caxes]), ptr(caxes_d), ptr(mean), ptr(var))

    def _predict_axes(self, o, taxes, mean, var):
        """The posterior on the product grid of the d coordinate vectors taxes, in the grid's own (C) order."""
        C = self.C
        shape = [len(t) for t in taxes]
        if int(np.prod(shape, dtype=np.int64)) != mean.shape[0]:
            raise NotImplementedError("solver='columns' predicts on product grids: %d test rows do not fill a grid of shape %s"
                                      % (mean.shape[0], tuple(shape)))
        rows = np.array(np.meshgrid(*[taxes[i] for i in C["ragged"]], indexing="ij")).reshape(len(C["ragged"]), -1).T
        mp, vp = torch.empty_like(mean), torch.empty_like(var)
        rc = self._predict_product(o, o._to_device(np.ascontiguousarray(rows)), [taxes[i] for i in C["complete"]], mp, vp)
        pshape = [shape[i] for i in C["perm"]]
        mean.copy_(mp.reshape(pshape).permute(C["inv"]).reshape(-1))
        var.copy_(vp.reshape(pshape).permute(C["inv"]).reshape(-1))
        return rc

    def predict_grid(self, o, mean, var):
        if self.taxes is not None:
            return self._predict_axes(o, self.taxes, mean, var)
        # no test grid: the training points, (observed ragged points) x (complete axes), back in their row-major order
        C = self.C
        if self._train_order is None:
            Ns, J = C["Y"].shape
            rshape = [C["shape"][i] for i in C["ragged"]]
            P = np.full((int(np.prod(rshape)), J), -1, dtype=np.int64)
            P[C["obs"]] = np.arange(Ns * J).reshape(Ns, J)
            P = P.reshape([C["shape"][i] for i in C["perm"]]).transpose(C["inv"]).ravel()
            self._train_order = torch.from_numpy(P[P >= 0]).to(o._dev)
        mp, vp = torch.empty_like(mean), torch.empty_like(var)
        rc = self._predict_product(o, self.Xs_d, C["axes_c"], mp, vp)
        torch.index_select(mp, 0, self._train_order, out=mean)
        torch.index_select(vp, 0, self._train_order, out=var)
        return rc

    def predict(self, o, Xs, mean, var):
        """Arbitrary rows, in any order, are served when they are (a set of ragged points) x (a product of coordinate vectors
        for the complete axes): every block then shares the complete axes' cross-covariances.  Rows with a NaN give NaN."""
        C = self.C
        X = Xs.cpu().numpy()[:, C["perm"]]
        p = len(C["ragged"])
        fin = np.isfinite(X).all(axis=1)
        Xf = X[fin]
        rows, ridx = np.unique(Xf[:, :p], axis=0, return_inverse=True)
        caxes, cidx = [], np.zeros(len(Xf), dtype=np.int64)
        for k in range(p, X.shape[1]):
            vals, inv = np.unique(Xf[:, k], return_inverse=True)
            caxes.append(vals)
            cidx = cidx * len(vals) + inv
        Mc = int(np.prod([len(c) for c in caxes], dtype=np.int64))
        flat = ridx.reshape(-1) * Mc + cidx
        if len(Xf) == 0 or len(rows) * Mc != len(Xf) or len(np.unique(flat)) != len(Xf):
            raise NotImplementedError("solver='columns' predicts on product test grids: the %d test rows are not (a set of "
                                      "points of the ragged axes %s) x (a product of coordinate vectors for the complete axes "
                                      "%s)" % (len(Xf), C["ragged"], C["complete"]))
        mp = torch.empty(len(Xf), dtype=_F64, device=o._dev)
        vp = torch.empty_like(mp)
        rc = self._predict_product(o, o._to_device(np.ascontiguousarray(rows)), caxes, mp, vp)
        flat_d = torch.from_numpy(flat).to(o._dev)
        if fin.all():
            torch.index_select(mp, 0, flat_d, out=mean)
            torch.index_select(vp, 0, flat_d, out=var)
        else:
            fin_d = torch.from_numpy(fin).to(o._dev)
            mean.fill_(float("nan"))
            var.fill_(float("nan"))
            mean[fin_d] = mp[flat_d]
            var[fin_d] = vp[flat_d]
        return rc

    def sample_geometry(self, taxes):
        """What a draw on the product grid of the d coordinate vectors taxes needs beside z: the ragged test rows (as
        ``_predict_axes`` builds them), the complete test axes, the union of the ragged rows and of the complete axes."""
        C = self.C
        rows = np.array(np.meshgrid(*[taxes[i] for i in C["ragged"]], indexing="ij")).reshape(len(C["ragged"]), -1).T
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        caxes = [np.asarray(taxes[i], dtype=np.float64) for i in C["complete"]]
        return rows, caxes, gprutils.union_rows(C["Xs"], rows), gprutils.union_axes(C["axes_c"], caxes)

    def sample_columns(self, o, taxes, z, noiseless, jitter, mean, out, geometry=None):
        """Joint posterior draws on the product grid of the axes ``taxes`` by Matheron's rule through the dense-by-Kronecker
        blocks (csrc/pkrongp.hip: gpimhip_sample_pkron).  z: (S, U_s prod U_i + N + M) device tensor
        [zeta | z_e | z_n], z_e in the training points' row order and z_n in the test grid's own (C) order; mean (M) and out
        (S, M) come back in the test grid's order."""
        C = self.C
        rows, caxes, (P, iX, iT), (au, ic, it) = geometry or self.sample_geometry(taxes)
        shape = [len(t) for t in taxes]
        N, M, S = C["n_obs"], int(np.prod(shape, dtype=np.int64)), z.shape[0]
        PU = z.shape[1] - N - M
        e_idx, n_idx, o_idx = (torch.from_numpy(a).to(o._dev) for a in gprutils.column_sample_maps(C, shape))
        zl = torch.empty_like(z)
        zl[:, :PU] = z[:, :PU]
        zl[:, PU:PU + N] = z[:, PU:PU + N].index_select(1, e_idx)
        zl[:, PU + N:] = z[:, PU + N:].index_select(1, n_idx)
        i32 = lambda v: (ctypes.c_int32 * len(v))(*[int(k) for k in v])
        # (every device tensor stays referenced until the call returns)
        rows_d, caxes_d, P_d, au_d = (o._to_device(a) for a in (rows, np.concatenate(caxes), P, np.concatenate(au)))
        mp, op = torch.empty_like(mean), torch.empty_like(out)
        rc = o._handle.lib.gpimhip_sample_pkron(*self._model(o), ptr(o._u), ptr(rows_d), rows_d.shape[0],
                                                i32([len(c) for c in caxes]), ptr(caxes_d), ptr(P_d), P_d.shape[0], i32(iX),
                                                i32(iT), i32([len(a) for a in au]), ptr(au_d), i32(np.concatenate(ic)),
                                                i32(np.concatenate(it)), ptr(zl), S, int(bool(noiseless)), float(jitter),
                                                ptr(mp), ptr(op))
        mean.copy_(mp.index_select(0, o_idx))
        out.copy_(op.index_select(1, o_idx))
        return rc


class Reflection(Dense):
    """Exact GP on a complete grid through its reflection blocks: 2^r dense blocks in one lock-step batch with shared
    hyper-parameters (gprutils.reflection_blocks; csrc/engine.hip: kmat_refl_kernel).  With ``border``: the blocks of the
    completed grid plus a border for its missing points (gprutils.border_blocks; csrc/border.hip)."""
    symm = True
    no_ivr = "the cross-covariance of arbitrary grid points is not block-structured"
    no_loo_objective = ("structured=True (reflection blocks): a held-out term mixes the diagonals of all blocks that hold its "
                        "point, so the objective is no sum over the blocks and the lock-step batch has no gradient for it")

    def __init__(self, S, border=False):
        self.S, self.border, self.blocks, self.perm_d = S, border, None, None
        self.rep32 = self.sgn32 = None                  # the index maps of loo(), uploaded on first use

    @contextlib.contextmanager
    def _mode(self, o, var_count=0):
        """The handle in reflection mode (with the border when there is one) for the body of the ``with``; yields the device
        side of the blocks, which go to the device on first use."""
        if self.blocks is None:
            self.blocks = DeviceBlocks(self.S, o._dev)
        D = self.blocks
        if self.border and D.border is None:
            D.upload_border()
        with _lib.reflection(o._handle, D, var_count, D.border):
            yield D

    def _call(self, o, fn, *args, var_count=0):
        """fn(h, model, Xq, 0, ys, Nq, B, u_b, *args) with the handle in reflection mode; the B parameter slots hold one
        vector, and the first comes back into ``o._u``."""
        with self._mode(o, var_count) as D:
            u_b = o._u.repeat(D.B).contiguous()
            rc = fn(*_head(o), ptr(D.Xq), 0, ptr(D.ys), D.Xq.shape[0], D.B, ptr(u_b), *args)
        o._u.copy_(u_b[:o._u.numel()])
        return rc

    def fit(self, o, lr, T, hist, loss):
        hist_b = torch.empty((self.S["B"],) + hist.shape, dtype=_F64, device=o._dev)
        loss_b = torch.empty((self.S["B"],) + loss.shape, dtype=_F64, device=o._dev)
        rc = self._call(o, o._handle.lib.gpimhip_fit_exact_batched, lr, T, ptr(hist_b), ptr(loss_b))
        hist.copy_(hist_b[0])                           # every slot holds the same history
        loss.copy_(loss_b[0])
        return rc

    def predict(self, o, Xs, mean, var, var_count=0):
        return self._call(o, o._handle.lib.gpimhip_predict_exact_batched, ptr(Xs), Xs.shape[0], ptr(mean), ptr(var),
                          var_count=var_count)

    def predict_grid(self, o, mean, var):
        Xt, S = o._Xtest_d, self.S
        if self.border or Xt.shape != o._Xd.shape or not bool(torch.equal(Xt, o._Xd)):
            return self.predict(o, Xt, mean, var)
        # the training grid itself: the variance is invariant under the reflections -- computed on the fundamental
        # domain (ordered first) and mirrored; the mean everywhere
        M, nq = Xt.shape[0], len(S["fund_flat"])
        if self.perm_d is None:
            rest = np.setdiff1d(np.arange(M), S["fund_flat"], assume_unique=True)
            self.perm_d = torch.from_numpy(np.concatenate([S["fund_flat"], rest])).to(o._dev)
            self.rep_d = torch.from_numpy(S["rep"]).to(o._dev)
        Xp = Xt[self.perm_d].contiguous()
        mean_p, var_p = torch.empty_like(mean), torch.empty_like(var)
        rc = self.predict(o, Xp, mean_p, var_p, var_count=nq)
        mean[self.perm_d] = mean_p
        torch.index_select(var_p[:nq], 0, self.rep_d, out=var)
        return rc

    def loo(self, o, mean, var, score):
        """The blocks' diagonals in one launch, combined in grid space with the weights |Stab_p| / B and the characters
        chi_s(sgn_i) (csrc/api.hip: gpimhip_loo_exact_batched).  The training rows are the complete grid in its order."""
        if self.border:
            self._loo_refused("with a border the missing points couple the reflection blocks, and diag(S^-1) is no longer a "
                              "weighted sum of the blocks' diagonals")
        self._loo_double_only(o)
        with self._mode(o) as D:
            if self.rep32 is None:
                i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(o._dev)
                self.rep32, self.sgn32 = i32(self.S["rep"]), i32(self.S["sgn"])
            u_b = o._u.repeat(D.B).contiguous()
            return o._handle.lib.gpimhip_loo_exact_batched(*_head(o), ptr(D.Xq), 0, ptr(D.ys), D.Xq.shape[0], D.B, ptr(u_b),
                                                           ctypes.c_void_p(self.rep32.data_ptr()),
                                                           ctypes.c_void_p(self.sgn32.data_ptr()), ptr(o._yd), ptr(mean),
                                                           ptr(var), ptr(score))

    def sample_border(self, o, Xs, P, miss_d, z, noiseless, jitter, mean, out):
        """Pathwise draws on the completed grid whose rows are Xs for a model with missing points, through the state a
        prediction of the bordered blocks leaves (csrc/sample.hip).  P: shape, mask and twoc of the
        completed grid; miss_d: the flat grid indices of the missing points on the device (int64, the border's order);
        z: (S, 2 M [+ M]), every part indexed by the grid point."""
        if not self.border:
            return Dense.sample_border(self, o)
        d = o._spec.dim
        shape = (ctypes.c_int32 * d)(*[int(n) for n in P["shape"]])
        twoc = (ctypes.c_double * 4)(*P["twoc"])
        return self._call(o, o._handle.lib.gpimhip_sample_border, ptr(Xs), shape, int(P["mask"]), twoc,
                          ctypes.c_void_p(miss_d.data_ptr()), ptr(z), z.shape[0], int(bool(noiseless)), float(jitter), ptr(mean),
                          ptr(out))

    def nll_grad(self, o, out):
        if not self.border:         # the dense model of the same data
            return Dense.nll_grad(self, o, out)
        # the coupled blocks with the border: one evaluation of what a training iteration computes
        return self._call(o, o._handle.lib.gpimhip_nll_grad_batched, *_loss_grad(out))


class SpectralBlocks(Reflection):
    """The spectral-mixture GP of ``smreconstructor`` on the reflection blocks of a complete grid, or of a completed one with
    a border (csrc/sm.hip: sm_kmat_refl_kernel, sm_grad_refl_kernel).  The blocks share ONE parameter
    vector ``o._u``; S["ones"] = U 1 (U 1_o with a border) carries the constant mean into the blocks.  ``predict_grid`` is
    Reflection's: on the training grid of a complete model the variance is computed on the fundamental domain."""

    def _call(self, o, fn, *args, var_count=0):
        """fn(h, sm, Xq, ys, ones, Nq, B, *args) with the handle in reflection mode."""
        with self._mode(o, var_count) as D:
            if D.ones is None:
                D.ones = D._up(self.S["ones"])
            return fn(o._handle.h, ctypes.byref(o._sstruct), ptr(D.Xq), ptr(D.ys), ptr(D.ones), D.Xq.shape[0], D.B, *args)

    def fit(self, o, lr, T, hist, loss):
        return self._call(o, o._handle.lib.gpimhip_fit_sm_batched, ptr(o._u), lr, T, ptr(hist), ptr(loss))

    def predict(self, o, Xs, mean, var, var_count=0):
        return self._call(o, o._handle.lib.gpimhip_predict_sm_batched, ptr(o._u), ptr(Xs), Xs.shape[0], ptr(mean), ptr(var),
                          var_count=var_count)

    def nll_grad(self, o, u, loss, grad):
        return self._call(o, o._handle.lib.gpimhip_sm_nll_grad_batched, ptr(u), ptr(loss), ptr(grad))
