"""The paired step schedule of the Cholesky (cholstep.hip: two block columns per step launch in the bulk regime, from 68 block
columns, for at most four problems) on the GPU: gpimhip_nll_grad and gpimhip_predict_exact against the oracle at sizes whose
plans have bulk panels (tests/test_step_plan_paired.py replays the same plans on the host):

  N = 9728  nb = 76: three bulk panels (six pair launches), then the per-column schedule;
  N = 9800  nb = 77: the same with a partial last block (72 valid rows, identity padding below);
  N = 9216  nb = 72, B = 2: a lock-step batch through the same launches, bit-equal to the single problems.

Tolerances and their derivation are those of test_gpu_regimes.py::test_lookahead_regime_vs_oracle: mid-range noise (u = -3)
keeps K's condition number moderate; the loss gets 1e-12 or 32x the oracle's own sensitivity to the order of the
observations (never more than 1e-10), the gradient rel 1e-10, the posterior abs 1e-10.  With the seeds below the oracle's
sensitivity, measured on the CPU, is 1.7e-14 at both sizes: 32x that is far below the 1e-10 cap, and the bar is 1e-12.

The per-column schedule (GPIMHIP_NO_PAIR_STEPS=1, read when a handle builds its plans) runs in a fresh child process and is
held to the same tolerances against the paired result."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from numpy.testing import assert_allclose

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M_TEST = 700


def problem(N, seed):
    """N random 2-D points in [0, 127]^2, a smooth signal plus noise, 700 test points (one NaN row)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 127.0, size=(N, 2))
    y = np.sin(X[:, 0] / 9.0) * np.cos(X[:, 1] / 13.0) + 0.1 * rng.standard_normal(N)
    Xs = rng.uniform(0.0, 127.0, size=(M_TEST, 2))
    Xs[11] = np.nan
    return torch.from_numpy(X), torch.from_numpy(y), torch.from_numpy(Xs)


def model(seed=0):
    from oracle import gpim_oracle as O
    from gpim_amd.kernels import KernelSpec
    ls = [[1., 1.], [20., 20.]]
    torch.manual_seed(seed)
    kp = O.KernelParams("Matern52", 2, ls)
    spec = KernelSpec("Matern52", 2, ls, jitter=1e-5)
    u = spec.draw_initial_u(torch.Generator().manual_seed(seed))
    with torch.no_grad():
        kp.u_noise.fill_(-3.0)
    u[1 + spec.n_ls] = -3.0
    return kp, spec, u


def engine_eval(N, seed):
    """loss + gradient, posterior mean and variance from the engine: four numpy arrays"""
    from gpim_amd import _lib
    X, y, Xs = problem(N, seed)
    _, spec, u = model()
    m = spec.struct()
    H = _lib.Handle()
    Xd, yd, ud, Xsd = X.cuda().contiguous(), y.cuda().contiguous(), u.cuda(), Xs.cuda().contiguous()
    out = torch.empty(1 + spec.n_params, dtype=torch.float64, device="cuda")
    _lib.check(H.lib.gpimhip_nll_grad(H.h, ctypes.byref(m), _lib.ptr(Xd), _lib.ptr(yd), N, _lib.ptr(ud),
                                      ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(out.data_ptr() + 8)))
    mean = torch.empty(M_TEST, dtype=torch.float64, device="cuda")
    var = torch.empty_like(mean)
    _lib.check(H.lib.gpimhip_predict_exact(H.h, ctypes.byref(m), _lib.ptr(Xd), _lib.ptr(yd), N, _lib.ptr(ud),
                                           _lib.ptr(Xsd), M_TEST, _lib.ptr(mean), _lib.ptr(var)))
    o = out.cpu().numpy()
    H.close()
    return o[:1].copy(), o[1:].copy(), mean.cpu().numpy(), var.cpu().numpy()


def oracle_eval(N, seed):
    from oracle import gpim_oracle as O
    from problems import oracle_threads
    from test_gpu_regimes import _loss_rtol
    X, y, Xs = problem(N, seed)
    kp, _, _ = model()
    with oracle_threads():
        gp = O.ExactGP(X, y, kp, 1e-5)
        loss_ref, g_ref = gp.loss_and_grad()
        mref, vref = gp.predict(Xs)
        with torch.no_grad():
            rtol, sens = _loss_rtol(lambda Xp, yp: O.ExactGP(Xp, yp, kp, 1e-5).loss().item(), X, y, loss_ref.item())
    assert 32.0 * sens < 1e-10, "the seed's problem is too ill-conditioned for the loss bar: change the seed"
    return loss_ref.item(), g_ref.numpy(), mref.numpy(), vref.numpy(), rtol, sens


def held_to(got, ref, rtol, what):
    loss, grad, mean, var = got
    loss_ref, g_ref, mref, vref = ref
    print("%s: loss rel. diff %.2e (bar %.2e), gradient %.2e, mean %.2e, variance %.2e" % (
        what, abs(loss[0] - loss_ref) / abs(loss_ref), rtol, np.abs(grad - g_ref).max() / np.abs(g_ref).max(),
        np.nanmax(np.abs(mean - mref)), np.nanmax(np.abs(var - vref))))
    assert_allclose(loss[0], loss_ref, rtol=rtol)
    assert_allclose(grad, g_ref, rtol=1e-10, atol=1e-10 * np.abs(g_ref).max())
    assert np.isnan(mean[11]) and np.isnan(var[11])
    ok = ~np.isnan(mref)
    assert_allclose(mean[ok], mref[ok], rtol=0, atol=1e-10)
    assert_allclose(var[ok], vref[ok], rtol=0, atol=1e-10)


@pytest.fixture(scope="module")
def paired_9728(ensure_built):
    assert "GPIMHIP_NO_PAIR_STEPS" not in os.environ
    return engine_eval(9728, 3), oracle_eval(9728, 3)


def test_pair_steps_vs_oracle(paired_9728):
    """nb = 76: six pair launches, the first per-column launch after a pair, then the chain-bound schedule."""
    got, ref = paired_9728
    held_to(got, ref[:4], ref[4], "paired, N = 9728")


def test_per_column_switch_in_a_fresh_process(paired_9728, tmp_path):
    """GPIMHIP_NO_PAIR_STEPS=1: the per-column schedule, against the paired result at the oracle's tolerances (and against the
    oracle itself)."""
    got, ref = paired_9728
    out = str(tmp_path / "percol.npz")
    code = ("import sys, numpy as np; sys.path[:0] = [%r, %r]; import test_gpu_pair_steps as t; "
            "l, g, m, v = t.engine_eval(9728, 3); np.savez(%r, l=l, g=g, m=m, v=v)" % (ROOT, os.path.join(ROOT, "tests"), out))
    env = dict(os.environ, GPIMHIP_NO_PAIR_STEPS="1")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]
    z = np.load(out)
    percol = (z["l"], z["g"], z["m"], z["v"])
    held_to(percol, ref[:4], ref[4], "per column, N = 9728")
    held_to(got, (percol[0][0], percol[1], percol[2], percol[3]), ref[4], "paired against per column")
    # the two schedules eliminate in a different order: had the switch not taken, the results would be the same bits
    assert not np.array_equal(got[2][~np.isnan(got[2])], percol[2][~np.isnan(percol[2])])


def test_pair_steps_ragged_last_block_vs_oracle(ensure_built):
    """N = 9800: nb = 77, the last block holds 72 valid rows; the pairs' strips run over its identity padding."""
    got = engine_eval(9800, 5)
    ref = oracle_eval(9800, 5)
    held_to(got, ref[:4], ref[4], "paired, N = 9800")


def test_pair_steps_batch_of_two_equals_single(ensure_built):
    """B = 2 at nb = 72 (N = 9216), two problems with their own observations and hyper-parameters on one set of points, in
    lock-step through the pair launches (gpimhip_predict_exact_batched: kernel matrix, factorisation + inverse, posterior):
    bit-equal to the problems one at a time -- the invariant of test_gpu_fused_predict.py at small N."""
    from gpim_amd import _lib
    N, B = 9216, 2
    X, y, Xs = problem(N, 9)
    _, spec, u = model()
    rng = np.random.default_rng(1)
    Y = torch.stack([y, torch.from_numpy(np.cos(X[:, 0].numpy() / 7.0) + 0.1 * rng.standard_normal(N))])
    U = torch.stack([u, u + 0.1])
    m = spec.struct()
    H = _lib.Handle()
    Xd, Yd, Ud, Xsd = X.cuda().contiguous(), Y.cuda().contiguous(), U.cuda().contiguous(), Xs.cuda().contiguous()
    mean = torch.empty(B, M_TEST, dtype=torch.float64, device="cuda")
    var = torch.empty_like(mean)
    _lib.check(H.lib.gpimhip_predict_exact_batched(H.h, ctypes.byref(m), _lib.ptr(Xd), 0, _lib.ptr(Yd), N, B,
                                                   _lib.ptr(Ud), _lib.ptr(Xsd), M_TEST, _lib.ptr(mean), _lib.ptr(var)))
    mean, var = mean.cpu().numpy(), var.cpu().numpy()
    H.close()
    H1 = _lib.Handle()
    for b in range(B):
        yd, ud = Y[b].cuda().contiguous(), U[b].cuda().contiguous()
        mb = torch.empty(M_TEST, dtype=torch.float64, device="cuda")
        vb = torch.empty_like(mb)
        _lib.check(H1.lib.gpimhip_predict_exact(H1.h, ctypes.byref(m), _lib.ptr(Xd), _lib.ptr(yd), N, _lib.ptr(ud),
                                                _lib.ptr(Xsd), M_TEST, _lib.ptr(mb), _lib.ptr(vb)))
        assert np.isfinite(np.delete(mean[b], 11)).all()
        assert np.array_equal(mean[b], mb.cpu().numpy(), equal_nan=True)
        assert np.array_equal(var[b], vb.cpu().numpy(), equal_nan=True)
    H1.close()
