"""
One acquisition formula (csrc/acq.hpp: acq_value) behind every sweep, on the MI355X: the map of gpimhip_acquire_exact -- the
epilogue of the fused launch at N = 40 (one block), acq_from_var_kernel behind the slab path at N = 530 (np = 640, 18 valid
rows in the last block) -- and round 0 of gpimhip_acquire_batch (CB) must be, bit for bit, gpimhip_acq (acq_kernel, the copy
the reference's goldens pin) of the same call's mean_out and sd_out.  For EI / POI the incumbent handed to gpimhip_acq is
recomputed outside the entry: gpimhip_predict_exact at the observed rows (the training rows), then gpimhip_nanmax over the
means (EI) or the means and the sds (POI).  M = 300 candidates on a 20 x 15 grid, with and without a 1 / NaN mask.
np.array_equal(..., equal_nan=True) throughout: there is no tolerance to choose.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ivr_oracle as IO

SHAPE = (20, 15)
PARAMS = {"cb": (1.0, 2.0), "ei": (0.0, 0.01), "poi": (0.0, 0.01)}        # (alpha, beta) or (ignored, xi)
CASES = [(N, masked) for N in (40, 530) for masked in (False, True)]
IDS = ["N%d%s" % (N, "-mask" if masked else "") for N, masked in CASES]


@pytest.fixture(scope="module")
def eng(ensure_built):
    from gpim_amd import _lib
    H = _lib.Handle()
    yield _lib, H
    H.close()


@pytest.fixture(scope="module")
def problems():
    """N -> (model struct, X, y, u, G) on the device, built once"""
    out = {}
    for N in (40, 530):
        _, spec, u, X, y, G = IO.case("Matern52", N, SHAPE)
        out[N] = (spec.struct(), X.cuda().contiguous(), y.cuda().contiguous(), u.cuda(), G.cuda().contiguous())
    return out


def mask_of(M, masked):
    if not masked:
        return None
    return torch.from_numpy(np.where(np.random.default_rng(3).uniform(size=M) < 0.25, np.nan, 1.0)).cuda()


def vec(n, dtype=torch.float64):
    return torch.empty(n, dtype=dtype, device="cuda")


def sweep(_lib, H, kind, mean, sd, p0, p1, mask):
    out = vec(mean.numel())
    _lib.check(H.lib.gpimhip_acq(H.h, _lib.ACQ_IDS[kind], _lib.ptr(mean), _lib.ptr(sd), mean.numel(), float(p0), float(p1),
                                 _lib.ptr(mask), _lib.ptr(out)))
    return out.cpu().numpy()


def incumbent(_lib, H, kind, m, X, y, u):
    """nanmax of the posterior at the training rows through the public entries: the means (EI), the means and sds (POI)"""
    N = X.shape[0]
    mean, var, best = vec(N), vec(N), vec(1)
    _lib.check(H.lib.gpimhip_predict_exact(H.h, ctypes.byref(m), _lib.ptr(X), _lib.ptr(y), N, _lib.ptr(u), _lib.ptr(X), N,
                                           _lib.ptr(mean), _lib.ptr(var)))
    t = mean if kind == "ei" else torch.cat([mean, var.sqrt()])
    _lib.check(H.lib.gpimhip_nanmax(H.h, _lib.ptr(t), t.numel(), _lib.ptr(best)))
    return best.item()


@pytest.mark.parametrize("kind", ["cb", "ei", "poi"])
@pytest.mark.parametrize("N,masked", CASES, ids=IDS)
def test_acquire_exact_is_acq_of_its_own_posterior(eng, problems, N, masked, kind):
    _lib, H = eng
    m, X, y, u, G = problems[N]
    M = G.shape[0]
    mask = mask_of(M, masked)
    p0, p1 = PARAMS[kind]
    acq, mean, sd = vec(M), vec(M), vec(M)
    _lib.check(H.lib.gpimhip_acquire_exact(H.h, ctypes.byref(m), _lib.ptr(X), _lib.ptr(y), N, _lib.ptr(u), _lib.ptr(G), M,
                                           _lib.ptr(X), N, _lib.ACQ_IDS[kind], p0, p1, _lib.ptr(mask), _lib.ptr(mean),
                                           _lib.ptr(sd), _lib.ptr(acq)))
    a = p0 if kind == "cb" else incumbent(_lib, H, kind, m, X, y, u)
    want = sweep(_lib, H, kind, mean, sd, a, p1, mask)
    got = acq.cpu().numpy()
    differ = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    print("%s N=%d mask=%s: a = %r, %d of %d entries differ, %d NaN" % (kind, N, masked, a, differ.sum(), M, np.isnan(got).sum()))
    assert np.isfinite(got).sum() >= M // 2
    assert np.array_equal(got, want, equal_nan=True)


@pytest.mark.parametrize("N,masked", CASES, ids=IDS)
def test_believer_round_zero_is_acq_of_its_own_posterior(eng, problems, N, masked):
    _lib, H = eng
    m, X, y, u, G = problems[N]
    M = G.shape[0]
    mask = mask_of(M, masked)
    p0, p1 = PARAMS["cb"]
    maps, mean, sd, val = vec(M), vec(M), vec(M), vec(1)
    idx, count = vec(1, torch.int64), vec(1, torch.int64)
    _lib.check(H.lib.gpimhip_acquire_batch(H.h, ctypes.byref(m), _lib.ptr(X), _lib.ptr(y), N, _lib.ptr(u), _lib.ptr(G), M, None,
                                           0, _lib.ACQ_IDS["cb"], p0, p1, _lib.ptr(mask), 1, _lib.ptr(mean), _lib.ptr(sd),
                                           _lib.ptr(maps), None, _lib.ptr(idx), _lib.ptr(val), _lib.ptr(count)))
    want = sweep(_lib, H, "cb", mean, sd, p0, p1, mask)
    got = maps.cpu().numpy()
    differ = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    print("believer cb N=%d mask=%s: %d of %d entries differ, %d NaN" % (N, masked, differ.sum(), M, np.isnan(got).sum()))
    assert np.isfinite(got).sum() >= M // 2
    assert np.array_equal(got, want, equal_nan=True)
