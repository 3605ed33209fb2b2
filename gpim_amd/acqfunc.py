"""
acqfunc.py -- acquisition functions over the dense grid, evaluated on the GPU.

Mirror of the reference's gpim/gpbayes/acqfunc.py:11-92: same call
signatures and return values ``(acq, (mean, sd))`` as numpy arrays.  The element-wise sweep
(CB / EI / POI, ``Phi`` through erfc) and the incumbent ``nanmax`` run in libgpimhip
(gpimhip_acq, gpimhip_nanmax).  ``gpmodel`` is normally a ``gpim_amd.reconstructor``; any
object with ``predict(X, verbose=0) -> (mean, sd)`` works (its arrays are uploaded).

Reference quirk kept on purpose (the golden test_poi.npy depends on it): in
``probability_of_improvement`` the incumbent is the nanmax over BOTH the posterior means and
the posterior standard deviations at the observed points (acqfunc.py:86-88).
"""
import ctypes

import numpy as np
import torch

from . import _lib

_F64 = torch.float64
_handles = {}


def _handle_for(gpmodel):
    h = getattr(gpmodel, "_handle", None)
    if h is not None:
        return h
    dev = _lib.require_gpu()
    if dev.index not in _handles:
        _handles[dev.index] = _lib.Handle()
    return _handles[dev.index]


def _device_pred(gpmodel, X, handle):
    """predict -> numpy results plus device copies (reused from the reconstructor if it has them)."""
    if hasattr(gpmodel, "_last_pred"):
        gpmodel._last_pred = None
    mean, sd = gpmodel.predict(X, verbose=0)
    last = getattr(gpmodel, "_last_pred", None)
    if last is not None:
        return mean, sd, last[0], last[1]
    md = torch.as_tensor(np.ascontiguousarray(mean), dtype=_F64).reshape(-1).to(handle.device)
    sdd = torch.as_tensor(np.ascontiguousarray(sd), dtype=_F64).reshape(-1).to(handle.device)
    return mean, sd, md, sdd


def _sweep(handle, kind, md, sdd, p0, p1, shape):
    out = torch.empty_like(md)
    _lib.check(handle.lib.gpimhip_acq(handle.h, _lib.ACQ_IDS[kind], _lib.ptr(md), _lib.ptr(sdd), md.numel(),
                                      float(p0), float(p1), None, _lib.ptr(out)))
    return out.cpu().numpy().reshape(shape), out


def _nanmax(handle, *tensors):
    t = tensors[0] if len(tensors) == 1 else torch.cat([x.reshape(-1) for x in tensors])
    t = t.contiguous()
    out = torch.empty((1,), dtype=_F64, device=t.device)
    _lib.check(handle.lib.gpimhip_nanmax(handle.h, _lib.ptr(t), t.numel(), _lib.ptr(out)))
    return out.item()


# ------------------------------------------------------------------ device-resident path (boptimizer)
def acquisition_on_device(gpmodel, kind, X_full, X_sparse, p0=0.0, p1=1.0, xi=0.01, Xf_d=None, mask_d=None,
                          Xobs_d=None):
    """The three built-in acquisition functions for a ``gpim_amd.reconstructor`` surrogate WITHOUT leaving
    the GPU: returns device tensors (acq, mean, sd) over the flattened grid (acq already multiplied by
    ``mask_d`` when one is given).  Same arithmetic as the public functions below.  The incumbent of EI / POI --
    nanmax of the posterior at the observed points, which the reference obtains from a second predict over the
    whole NaN-masked grid (acqfunc.py:58-59,86-88) -- is predicted at the observed rows only: every column of a
    prediction is independent of the others, so the values (and their nanmax) are the same and the N^2 M
    triangular product shrinks to N^2 N_obs.  Exact models go through ONE library call (gpimhip_acquire_exact:
    one factorisation, incumbent kept on the device, fused posterior + acquisition launch for N <= 384).
    ``Xobs_d``: the observed rows of ``X_sparse`` when the caller already holds them on the device (boptimizer:
    they are the surrogate's training inputs)."""
    handle = gpmodel._handle
    Xf = Xf_d if Xf_d is not None else gpmodel._to_device(_rows(X_full, gpmodel.precision))
    Xobs = Xobs_d
    if kind != "cb" and Xobs is None:
        Xs = _rows(X_sparse, gpmodel.precision)
        obs = ~torch.isnan(Xs).any(dim=1)
        Xobs = gpmodel._to_device(Xs[obs].contiguous())
    if not gpmodel.do_sparse and not gpmodel.do_structured:
        gpmodel._check_data()
        M = Xf.shape[0]
        mean_d = torch.empty((M,), dtype=_F64, device=Xf.device)
        sd_d = torch.empty_like(mean_d)
        out = torch.empty_like(mean_d)
        a, b = (p0, p1) if kind == "cb" else (0.0, xi)
        _lib.check(handle.lib.gpimhip_acquire_exact(
            handle.h, ctypes.byref(gpmodel._mstruct), _lib.ptr(gpmodel._Xd), _lib.ptr(gpmodel._yd), gpmodel._Xd.shape[0],
            _lib.ptr(gpmodel._u), _lib.ptr(Xf), M, None if Xobs is None else _lib.ptr(Xobs),
            0 if Xobs is None else Xobs.shape[0], _lib.ACQ_IDS[kind], float(a), float(b),
            None if mask_d is None else _lib.ptr(mask_d), _lib.ptr(mean_d), _lib.ptr(sd_d), _lib.ptr(out)))
        return out, mean_d, sd_d
    mean_d, sd_d = gpmodel._predict_device(Xf)
    if kind == "cb":
        a, b = p0, p1
    else:
        mo, so = gpmodel._predict_device(Xobs)
        a = _nanmax(handle, mo) if kind == "ei" else _nanmax(handle, mo, so)
        b = xi
    out = torch.empty_like(mean_d)
    _lib.check(handle.lib.gpimhip_acq(handle.h, _lib.ACQ_IDS[kind], _lib.ptr(mean_d), _lib.ptr(sd_d), mean_d.numel(),
                                      float(a), float(b), None if mask_d is None else _lib.ptr(mask_d), _lib.ptr(out)))
    return out, mean_d, sd_d


def _rows(X, precision):
    from . import gprutils
    return gprutils.prepare_test_data(np.asarray(X), precision=precision)


def confidence_bound(gpmodel, X_full, **kwargs):
    """alpha * mean + beta * sd (defaults 0, 1)."""
    alpha, beta = kwargs.get("alpha", 0), kwargs.get("beta", 1)
    handle = _handle_for(gpmodel)
    mean, sd, md, sdd = _device_pred(gpmodel, X_full, handle)
    acq, acq_d = _sweep(handle, "cb", md, sdd, alpha, beta, mean.shape)
    gpmodel._last_acq = acq_d if hasattr(gpmodel, "_last_pred") else None
    return acq, (mean, sd)


def expected_improvement(gpmodel, X_full, X_sparse, **kwargs):
    """imp * Phi(imp/sd) + sd * phi(imp/sd), imp = mean - max(mean at observed points) - xi."""
    xi = kwargs.get("xi", 0.01)
    handle = _handle_for(gpmodel)
    mean, sd, md, sdd = _device_pred(gpmodel, X_full, handle)
    _, _, mo, _ = _device_pred(gpmodel, X_sparse, handle)     # NaN rows -> NaN means
    best = _nanmax(handle, mo)
    acq, acq_d = _sweep(handle, "ei", md, sdd, best, xi, mean.shape)
    gpmodel._last_acq = acq_d if hasattr(gpmodel, "_last_pred") else None
    return acq, (mean, sd)


def probability_of_improvement(gpmodel, X_full, X_sparse, **kwargs):
    """Phi((mean - incumbent - xi) / sd) with the reference's (mean, sd)-tuple incumbent."""
    xi = kwargs.get("xi", 0.01)
    handle = _handle_for(gpmodel)
    mean, sd, md, sdd = _device_pred(gpmodel, X_full, handle)
    _, _, mo, so = _device_pred(gpmodel, X_sparse, handle)
    best = _nanmax(handle, mo, so)
    acq, acq_d = _sweep(handle, "poi", md, sdd, best, xi, mean.shape)
    gpmodel._last_acq = acq_d if hasattr(gpmodel, "_last_pred") else None
    return acq, (mean, sd)


def thompson_on_device(gpmodel, Xf_d, generator=None, z=None, method='joint', grid_shape=None, n_draws=1):
    """Noiseless joint draws over the device rows ``Xf_d`` plus the posterior (mean, sd): device tensors (draw, mean, sd),
    ``draw`` of shape (M,) for one draw and (n_draws, M) for more.  ``z``: the standard normals, else drawn from
    ``generator`` (None: the global device generator) by the rule documented at ``reconstructor.sample``.
    ``method='joint'``: one library call gives all three.  ``method='pathwise'`` (``grid_shape``: the shape of the product
    grid the rows fill): the draws by Matheron's rule, (mean, sd) from the ordinary prediction."""
    if method == 'pathwise':
        if z is None:
            z = gpmodel._draw_z(n_draws, Xf_d.shape[0] + gpmodel._Xd.shape[0], generator=generator)
        draws, _ = gpmodel._sample_pathwise_device(Xf_d, grid_shape, z, noiseless=True)
        mean_d, sd_d = gpmodel._predict_device(Xf_d)
    elif method == 'joint':
        if z is None:
            z = gpmodel._draw_z(n_draws, Xf_d.shape[0], generator=generator)
        draws, mean_d, var_d = gpmodel._sample_device(Xf_d, z, noiseless=True)
        sd_d = var_d.sqrt()
    else:
        raise ValueError("method must be 'joint' or 'pathwise'; got %r" % (method,))
    return (draws[0] if draws.shape[0] == 1 else draws), mean_d, sd_d


def thompson_sampling(gpmodel, X_full, **kwargs):
    """Thompson sampling: the acquisition map is ONE joint draw from the noiseless posterior over the grid, so its
    maximiser is distributed like the maximiser of the unknown function.  kwargs: ``seed`` (int), ``generator`` (a device
    torch.Generator) or ``z`` ((1, M) standard normals; (1, M + N) for the pathwise method); none of them: the global
    device generator.  ``method``: 'joint' (default) or 'pathwise' (reconstructor.sample).  ``gpmodel`` is a dense
    double-precision ``gpim_amd.reconstructor``."""
    if not hasattr(gpmodel, "_sample_device"):
        raise NotImplementedError("thompson_sampling needs a gpim_amd.reconstructor (joint posterior draws)")
    Xf = gpmodel._to_device(_rows(X_full, gpmodel.precision))
    gen, z = kwargs.get("generator"), kwargs.get("z")
    if gen is None and z is None and kwargs.get("seed") is not None:
        gen = torch.Generator(gpmodel._dev).manual_seed(int(kwargs.get("seed")))
    if z is not None:
        z = gpmodel._to_device(z if torch.is_tensor(z) else np.asarray(z)).reshape(1, -1)
    shape = tuple(np.shape(X_full)[1:])
    acq_d, mean_d, sd_d = thompson_on_device(gpmodel, Xf, generator=gen, z=z, method=kwargs.get("method", "joint"),
                                             grid_shape=shape)
    gpmodel._last_acq = acq_d
    host = torch.stack([acq_d, mean_d, sd_d]).cpu().numpy().astype(gpmodel._np_out, copy=False)
    return host[0].reshape(shape), (host[1].reshape(shape), host[2].reshape(shape))


def _ivr_band(band, M):
    """``band`` of the ivr entries as what the solver hooks take: None (the M x M covariance is stored) or the number of
    128-column block columns of it held at a time.  None and an int >= 1 pass through.  'auto': None
    up to pad(M, 128) = 16384 -- the largest grid measured with the covariance stored -- and beyond it the widest band whose
    buffer stays within 2 GiB, ``max(1, 2**28 // (128 * pad(M, 128)))``: 32 at M = 65536, 8 at M = 262144.  ValueError for
    anything else.  A pure host function."""
    if band is None:
        return None
    if isinstance(band, str) and band == "auto":
        mp = -(-int(M) // 128) * 128
        return None if mp <= 16384 else max(1, 2 ** 28 // (128 * mp))
    if isinstance(band, (int, np.integer)) and not isinstance(band, bool) and band >= 1:
        return int(band)
    raise ValueError("ivr: band must be None, 'auto' or an int >= 1 (block columns of 128 held at a time); got %r" % (band,))


def ivr_on_device(gpmodel, Xf_d, weights_d=None, mask_d=None, band=None):
    """Integrated variance reduction (ALC) over the device rows ``Xf_d``: device tensors (acq, mean, sd) with
    ``acq[j] = sum_m w_m C_mj^2 / (max(C_jj, 0) + noise + jitter)``, C the latent posterior covariance of the rows -- how
    much the (weighted) total posterior variance of the rows drops when row j is measured -- and (mean, sd) the posterior of
    ``predict``.  ``weights_d``: (M,) device weights >= 0 of the integral (None: all 1); ``mask_d``: (M,) device mask of
    1 / NaN multiplied into ``acq`` (it excludes candidates, it does not change the integral).  One library call
    (gpimhip_ivr_exact).  ``band``: None, 'auto' or an int >= 1 (``_ivr_band``) -- the covariance in
    bands of that many block columns instead of M^2 doubles of device memory, the same map (gpimhip_ivr_exact_banded;
    section 30).  Dense double-precision models only; the rows must be finite."""
    M = _ivr_check_args(gpmodel, Xf_d, weights_d, mask_d)
    band = _ivr_band(band, M)
    mean_d = torch.empty((M,), dtype=_F64, device=Xf_d.device)
    sd_d = torch.empty_like(mean_d)
    acq_d = torch.empty_like(mean_d)
    _lib.check(gpmodel._solver.ivr(gpmodel, Xf_d, weights_d, mask_d, mean_d, sd_d, acq_d, band=band))
    return acq_d, mean_d, sd_d


def _ivr_check_args(gpmodel, Xf_d, weights_d, mask_d):
    """The checks of ``ivr_on_device`` and ``ivr_greedy_on_device``; returns the number of rows."""
    gpmodel._check_data()
    if not bool(torch.isfinite(Xf_d).all()):
        raise ValueError("ivr: the test grid must be finite (NaN / inf rows have no covariance with the others)")
    M = Xf_d.shape[0]
    for name, t in (("weights", weights_d), ("mask", mask_d)):
        if t is not None and (t.dim() != 1 or t.numel() != M or t.dtype != _F64 or not t.is_contiguous()):
            raise ValueError("ivr: %s must be a contiguous float64 device vector of %d entries" % (name, M))
    return M


def ivr_greedy_on_device(gpmodel, Xf_d, q, weights_d=None, mask_d=None, band=None):
    """A greedy batch of ``q`` picks by integrated variance reduction over the device rows ``Xf_d``: device tensors
    ``(idx, gain, count, maps, mean, sd, sd_after)``.  A GP's variance does not depend on the measured values, so pick r
    is the maximiser of the map of the covariance conditioned on picks 0 .. r - 1 (C <- C - c c^T / (C_pp + noise + jitter),
    c = C[:, p]): ``idx`` (q,) int64 flat indices in pick order, ``gain`` (q,) the map values -- the drop of the (weighted)
    total posterior variance each pick adds to the batch's -- ``count`` (1,) int64 the picks made (fewer than q when the
    unmasked candidates run out; then idx = -1 and gain = NaN behind them), ``maps`` (q, M) the map each pick was taken from
    (NaN at masked candidates and earlier picks; row 0 is ``ivr_on_device``'s map, bit for bit), ``mean``, ``sd`` the posterior
    before the batch, ``sd_after`` the sd once the batch is measured.  Arguments as ``ivr_on_device``; 1 <= q <= M.  One
    library call (gpimhip_ivr_greedy).  ``band`` as in ``ivr_on_device`` (gpimhip_ivr_greedy_banded):
    without the stored covariance a further pick costs a whole M^2 N product instead of one M^2 pass -- the price of the
    memory.  Dense double-precision models only."""
    M = _ivr_check_args(gpmodel, Xf_d, weights_d, mask_d)
    band = _ivr_band(band, M)
    q, out = _batch_outputs("ivr", q, M, Xf_d.device)
    idx_d, gain_d, count_d, maps_d, mean_d, sd_d, sd_after_d = out
    _lib.check(gpmodel._solver.ivr_greedy(gpmodel, Xf_d, weights_d, mask_d, q, mean_d, sd_d, maps_d, sd_after_d, idx_d,
                                          gain_d, count_d, band=band))
    return out


def _batch_outputs(who, q, M, dev):
    """``q`` as an int, checked (1 <= q <= M; ``who`` opens the message), and the seven device tensors a batch entry fills:
    ``(idx (q,) int64, val (q,), count (1,) int64 zero, maps (q, M), mean, sd, sd_after (M,))``."""
    q = int(q)
    if q < 1 or q > M:
        raise ValueError("%s: a batch of %d picks from %d candidates (1 <= q <= M)" % (who, q, M))
    mean_d, sd_d, sd_after_d = (torch.empty((M,), dtype=_F64, device=dev) for _ in range(3))
    maps_d = torch.empty((q, M), dtype=_F64, device=dev)
    val_d = torch.empty((q,), dtype=_F64, device=dev)
    idx_d = torch.empty((q,), dtype=torch.int64, device=dev)
    count_d = torch.zeros((1,), dtype=torch.int64, device=dev)
    return q, (idx_d, val_d, count_d, maps_d, mean_d, sd_d, sd_after_d)


def believer_on_device(gpmodel, kind, Xf_d, q, p0=0., p1=1., xi=0.01, mask_d=None, Xobs_d=None):
    """A believer batch of ``q`` picks for ``kind`` ('cb' / 'ei' / 'poi') over the device rows ``Xf_d``: device tensors
    ``(idx, val, count, maps, mean, sd, sd_after)``.  After each pick the model is conditioned on the pick having been
    measured at its posterior mean (kriging believer; GP-BUCB for 'cb'): the mean does not change, the variance drops as in
    ``ivr_greedy_on_device``, and the next pick maximises the acquisition function of the conditioned model -- two
    neighbouring maxima that explain the same pixels are not both taken.  ``idx`` (q,) int64 flat indices in pick order,
    ``val`` (q,) the map values at the picks, ``count`` (1,) int64 the picks made (fewer than q when the unmasked candidates
    run out; then idx = -1 and val = NaN behind them), ``maps`` (q, M) the map each pick was taken from (NaN at masked
    candidates and earlier picks), ``mean``, ``sd`` the posterior before the batch, ``sd_after`` the sd once the batch is
    measured.  ``p0``, ``p1``: alpha, beta of 'cb'; ``xi``: of 'ei' / 'poi', whose incumbent is the maximum of the posterior
    at the observed rows ``Xobs_d`` (default: the model's training inputs) and of the believed values.  ``mask_d``: (M,)
    device mask of 1 / NaN.  1 <= q <= M.  One library call (gpimhip_acquire_batch): one pass over
    W = L^-1 K(X, Xf) per pick, no M x M matrix.  Dense double-precision models only."""
    if kind not in _lib.ACQ_IDS:
        raise ValueError("acq_batch: the acquisition function must be 'cb', 'ei' or 'poi'; got %r" % (kind,))
    gpmodel._solver._believer_supported(gpmodel)
    M = _ivr_check_args(gpmodel, Xf_d, None, mask_d)
    q, out = _batch_outputs("acq_batch", q, M, Xf_d.device)
    idx_d, val_d, count_d, maps_d, mean_d, sd_d, sd_after_d = out
    if kind != "cb" and Xobs_d is None:
        Xobs_d = gpmodel._Xd
    a, b = (p0, p1) if kind == "cb" else (0.0, xi)
    _lib.check(gpmodel._solver.believer(gpmodel, kind, Xf_d, None if kind == "cb" else Xobs_d, a, b, mask_d, q, mean_d, sd_d,
                                        maps_d, sd_after_d, idx_d, val_d, count_d))
    return out


def _ivr_mask(mask, shape, dev):
    """``mask`` (None or an array of the grid's shape holding 1 / NaN) as a flat device vector."""
    if mask is None:
        return None
    k = np.asarray(mask, dtype=np.float64)
    if k.shape != tuple(shape):
        raise ValueError("ivr: mask must have the shape of the test grid %s; got %s" % (tuple(shape), k.shape))
    if not (np.isnan(k) | (k == 1.0)).all():
        raise ValueError("ivr: mask must hold 1 (a candidate) or NaN (excluded)")
    return torch.from_numpy(np.ascontiguousarray(k).reshape(-1)).to(dev)


def _ivr_weights(weights, shape, dev):
    """``weights`` (None or an array of the grid's shape, finite and >= 0) as a flat device vector."""
    if weights is None:
        return None
    w = np.asarray(weights, dtype=np.float64)
    if w.shape != tuple(shape):
        raise ValueError("ivr: weights must have the shape of the test grid %s; got %s" % (tuple(shape), w.shape))
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError("ivr: weights must be finite and >= 0")
    return torch.from_numpy(np.ascontiguousarray(w).reshape(-1)).to(dev)


def integrated_variance_reduction(gpmodel, X_full, X_sparse=None, **kwargs):
    """Integrated variance reduction (ALC): for every grid point, how much the total posterior variance of the whole grid
    drops when that point is measured.  kwargs: ``weights`` (array of the grid's shape, >= 0: the integral's weights),
    ``band`` (None, 'auto' or an int >= 1: the covariance in bands of block columns, as ``reconstructor.ivr``).
    ``X_sparse`` is not used (the signature of the other acquisition functions, so that this one also serves as a custom
    callable of ``boptimizer``).  ``gpmodel`` is a dense double-precision ``gpim_amd.reconstructor``."""
    if not hasattr(gpmodel, "_solver") or not hasattr(gpmodel._solver, "ivr"):
        raise NotImplementedError("integrated_variance_reduction needs a gpim_amd.reconstructor")
    shape = tuple(np.shape(X_full)[1:])
    Xf = gpmodel._to_device(_rows(X_full, gpmodel.precision))
    acq_d, mean_d, sd_d = ivr_on_device(gpmodel, Xf, _ivr_weights(kwargs.get("weights"), shape, gpmodel._dev),
                                        band=kwargs.get("band"))
    gpmodel._last_acq = acq_d
    host = torch.stack([acq_d, mean_d, sd_d]).cpu().numpy().astype(gpmodel._np_out, copy=False)
    return host[0].reshape(shape), (host[1].reshape(shape), host[2].reshape(shape))
