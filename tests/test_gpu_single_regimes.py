"""
The single-precision engine (csrc/cholstep32.hip, the float plan of csrc/cholstep.hip) at the smallest size of every
regime of its schedule, in lock-step batches, and at the edges of the prediction path -- held to the standard that
tests/test_gpu_regimes.py and tests/test_gpu_ops.py set for the double engine.

Hyper-parameters are set, not drawn (fixed_problem): variance 1, lengthscale 2 in every dimension, noise exp(-2) =
0.1353, alpha = 1 for RationalQuadratic, jitter 1e-5 -- so that the conditioning of K + (noise + jitter) I does not
grow with N (training points are distinct lattice points at density 1/4, a lengthscale covers a handful of them).  In
the unconstrained vector: u_var = logit((1 - 1e-4) / (10 - 1e-4)) = -2.1971, u_ls = logit((2 - 1) / (side - 1)) with
side the upper lengthscale bound of tests/test_gpu_single.py's problem(), u_noise = -2.

Oracle sizes (truth: the fp64 CPU oracle): the bars of test_single_engine_vs_truth_and_float32_run.

Engine-truth sizes (truth: the double-precision handle on the same inputs, itself held to the oracle at 8192 and 16384
in test_gpu_regimes.py / test_gpu_fullsize.py; independent float32 run: the double handle's covariance rounded to
float32, torch.linalg.cholesky and solve_triangular on the GPU in float32).  Launch shapes of launch_potrf_steps_f32
each size reaches (from the plan, gpimhip_step_plan_host_f32: hosted tiles per step launch, <= 128 quadrants, <= 512
halves, whole tiles beyond):

    N       block columns   step launches as quadrants / halves / whole tiles     launches before a panel (bulk_rest)
    6200         49                    33 / 16 /  0                                         none
    8200         65                    33 / 32 /  0                                         none
    8600         68                    33 / 31 /  4   (up to 521 tiles)                     none
    11200        88                    33 / 55 /  0   (bulk fill capped at 128)             13, up to 2728 tiles
    20400       160                    67 / 93 /  0   (bulk fill capped at 64, pair mode)   27, up to 10770 tiles

(8600 is not a policy boundary: it is the smallest size whose step launches reach the whole-tile shape -- 68 to 87
block columns do -- which none of the sizes above does.)

Measured on an MI355X (2026-10-17), error against the truth: engine / float32 run / bar.  The loss is relative, the
gradient relative to its largest component, mean and variance are the largest absolute difference over 500 points:

             loss (relative)      gradient   mean                 variance
    N        engine    float32    engine     engine    float32    engine    float32
    6200     9.3e-08   1.1e-07    2.4e-07    3.6e-08   2.9e-07    3.8e-07   4.1e-07
    8200     1.7e-07   1.2e-07    4.1e-07    5.1e-08   3.6e-07    4.1e-07   3.5e-07
    8600     9.3e-08   6.7e-08    2.5e-07    3.2e-08   3.3e-07    4.4e-07   5.8e-07
    11200    9.4e-08   2.0e-08    2.5e-07    2.9e-08   3.3e-07    4.7e-07   5.1e-07
    20400    9.6e-08   1.0e-07    2.6e-07    3.2e-08   2.8e-07    4.0e-07   5.5e-07
    bar      max(4 x float32, 2e-5)  5e-4    float32 + 1e-6       8 x float32 + 1e-6

The absolute bars of test_gpu_single.py (loss 5e-5, mean 2e-3 (max|mean| + 1), variance rtol 2e-2 / atol 1e-4) are
asserted as well.  The errors do not grow with N: the conditioning is held, and no tile is wrong or missing (that would be an
error of order one).

The gradient has no float32 run beside it; its bar is the project's 5e-4 of the largest component (test_gpu_single.py),
which every size meets by three orders of magnitude, so it stays.
"""
import ctypes
import math

import numpy as np
import pytest
import torch
from numpy.testing import assert_allclose

from oracle import gpim_oracle as O
from test_gpu_single import problem, run_engine, torch_float32_run

pytestmark = pytest.mark.gpu

JITTER = 1e-5
VARIANCE, LENGTHSCALE, U_NOISE = 1.0, 2.0, -2.0


@pytest.fixture(scope="module")
def lib(ensure_built):
    from gpim_amd import _lib
    return _lib


def fixed_problem(N, d, kind, seed, isotropic=False):
    """problem() of test_gpu_single.py with the constrained hyper-parameters set directly (module docstring), through
    the inverse of KernelSpec's interval map; the oracle's parameters hold the same u."""
    from gpim_amd.kernels import KernelSpec, _logit_clipped
    X, y, _, spec0, _, Xs = problem(N, d, kind, seed)
    lo, hi = spec0.ls_lo.tolist(), spec0.ls_hi.tolist()
    ls = [lo[0], hi[0]] if isotropic else [lo, hi]
    kp = O.KernelParams(kind, d, ls)
    spec = KernelSpec(kind, d, ls, jitter=JITTER)
    f64 = torch.float64
    u = torch.zeros(spec.n_params, dtype=f64)
    u[0] = _logit_clipped(torch.tensor((VARIANCE - spec.amp_lo) / (spec.amp_hi - spec.amp_lo), dtype=f64))
    u[1:1 + spec.n_ls] = _logit_clipped((LENGTHSCALE - spec.ls_lo) / (spec.ls_hi - spec.ls_lo))
    u[1 + spec.n_ls] = U_NOISE
    with torch.no_grad():
        kp.u_var.copy_(u[0])
        kp.u_ls.copy_(u[1:1 + spec.n_ls].reshape(kp.u_ls.shape))
        kp.u_noise.fill_(U_NOISE)
    var, lsv, noise = spec.constrained(u)
    assert abs(var.item() - VARIANCE) < 1e-12 and (lsv - LENGTHSCALE).abs().max() < 1e-12
    assert abs(kp.variance.item() - VARIANCE) < 1e-12 and abs(kp.noise.item() - math.exp(U_NOISE)) < 1e-15
    return X, y, kp, spec, u, Xs


def oracle_truth(X, y, kp, Xs):
    gp = O.ExactGP(torch.from_numpy(X), torch.from_numpy(y), kp, JITTER)
    loss, grad = gp.loss_and_grad()
    mean, var = (t.numpy() for t in gp.predict(torch.from_numpy(Xs)))
    return loss.item(), grad.numpy(), mean, var


def assert_bars(got, truth, tag=""):
    """The bars of test_single_engine_vs_truth_and_float32_run against the truth."""
    loss, grad, mean, var = got
    loss_t, grad_t, mean_t, var_t = truth
    print("%s vs truth: loss rel %.2e, grad / max|grad| %.2e, mean %.2e, var %.2e" % (
        tag, abs(loss - loss_t) / abs(loss_t), np.abs(grad - grad_t).max() / np.abs(grad_t).max(),
        np.abs(mean - mean_t).max(), np.abs(var - var_t).max()))
    assert_allclose(loss, loss_t, rtol=5e-5)
    assert_allclose(grad, grad_t, rtol=0, atol=5e-4 * np.abs(grad_t).max())
    assert_allclose(mean, mean_t, rtol=0, atol=2e-3 * (np.abs(mean_t).max() + 1))
    assert_allclose(var, var_t, rtol=2e-2, atol=1e-4)


def assert_ratios(got, f32, truth, tag=""):
    """Never further from the truth than a few times a plain float32 run of the same formulas."""
    loss, _, mean, var = got
    loss_f, mean_f, var_f = f32
    loss_t, _, mean_t, var_t = truth
    print("%s float32 run vs truth: loss rel %.2e, mean %.2e, var %.2e" % (
        tag, abs(loss_f - loss_t) / abs(loss_t), np.abs(mean_f - mean_t).max(), np.abs(var_f - var_t).max()))
    assert np.abs(mean - mean_t).max() <= np.abs(mean_f - mean_t).max() + 1e-6
    assert np.abs(var - var_t).max() <= 8 * np.abs(var_f - var_t).max() + 1e-6
    assert abs(loss - loss_t) <= max(4 * abs(loss_f - loss_t), 2e-5 * abs(loss_t))


def gpu_float32_run(lib, spec, u, X, y, Xs):
    """torch_float32_run of test_gpu_single.py on the GPU: the covariance from gpimhip_kmat on a double handle, rounded
    to float32, then float32 torch.linalg.cholesky / solve_triangular."""
    H = lib.Handle()
    try:
        N, M = len(X), len(Xs)
        var, ls, noise = spec.constrained(u)
        theta = torch.cat([var.reshape(1), ls.reshape(-1), torch.ones(1, dtype=torch.float64)]).cuda()
        m = spec.struct()
        Xd, Xsd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (X, Xs))
        K64 = torch.empty((N, N), dtype=torch.float64, device="cuda")
        lib.check(H.lib.gpimhip_kmat(H.h, ctypes.byref(m), lib.ptr(Xd), N, None, 0, lib.ptr(theta), 0.0, lib.ptr(K64), N))
        Ks64 = torch.empty((N, M), dtype=torch.float64, device="cuda")
        lib.check(H.lib.gpimhip_kmat(H.h, ctypes.byref(m), lib.ptr(Xd), N, lib.ptr(Xsd), M, lib.ptr(theta), 0.0,
                                     lib.ptr(Ks64), M))
        torch.cuda.synchronize()
        K = K64.float()
        del K64
        K.view(-1)[::N + 1] += float(JITTER + noise)
        L = torch.linalg.cholesky(K)
        del K
        z = torch.linalg.solve_triangular(L, torch.from_numpy(y).cuda().float().unsqueeze(-1), upper=False).squeeze(-1)
        prior = math.log(spec.amp_hi - spec.amp_lo) + float(torch.log(spec.ls_hi - spec.ls_lo).sum())
        loss = 0.5 * (z * z).sum() + L.diagonal().log().sum() + 0.5 * N * math.log(2 * math.pi) + prior
        W = torch.linalg.solve_triangular(L, Ks64.float(), upper=False)
        mean = W.t() @ z
        v = (float(var) - (W * W).sum(0)).clamp(min=0) + float(noise)
        out = float(loss), mean.double().cpu().numpy(), v.double().cpu().numpy()
        del L, W, Ks64
        return out
    finally:
        H.close()


ORACLE_SIZES = [("RBF", 100, 2, False), ("Matern52", 128, 2, False),          # one block
                ("RBF", 129, 2, False),                                        # one valid row in the last block
                ("Matern52", 448, 2, False), ("RBF", 449, 2, False),           # the boundary of the skipped padding
                ("Matern52", 530, 4, False), ("RBF", 300, 1, False),
                ("RationalQuadratic", 449, 2, True),                           # one isotropic lengthscale
                ("Matern52", 1207, 2, False)]
ENGINE_SIZES = [("Matern52", 6200), ("RBF", 8200), ("Matern52", 8600), ("Matern52", 11200), ("Matern52", 20400)]


@pytest.mark.parametrize("kind,N,d,isotropic", ORACLE_SIZES)
def test_float_schedule_vs_oracle(lib, kind, N, d, isotropic):
    X, y, kp, spec, u, Xs = fixed_problem(N, d, kind, seed=N, isotropic=isotropic)
    truth = oracle_truth(X, y, kp, Xs)
    H32 = lib.Handle(precision="single")
    try:
        got = run_engine(lib, H32, X, y, spec, u, Xs)
    finally:
        H32.close()
    assert_bars(got, truth, "N = %d" % N)
    assert_ratios(got, torch_float32_run(kp, X, y, Xs, JITTER), truth, "N = %d" % N)


@pytest.mark.parametrize("kind,N", ENGINE_SIZES)
def test_float_schedule_vs_double_engine(lib, kind, N):
    """49 / 65 / 68 block columns (everything hosted), 88 (capped fill, a launch before the panel's first step; 11200 =
    87 blocks + 64 rows), 160 (pair mode; 20400 = 159 blocks + 48 rows)."""
    X, y, kp, spec, u, Xs = fixed_problem(N, 2, kind, seed=N)
    got = truth = None
    for prec in ("double", "single"):
        H = lib.Handle(precision=prec)
        try:
            out = run_engine(lib, H, X, y, spec, u, Xs)
        finally:
            H.close()
        if prec == "double":
            truth = out
        else:
            got = out
    torch.cuda.empty_cache()
    assert_bars(got, truth, "N = %d" % N)
    f32 = gpu_float32_run(lib, spec, u, X, y, Xs)
    torch.cuda.empty_cache()
    assert_ratios(got, f32, truth, "N = %d" % N)


# ---------------------------------------------------------------------------------------------
# lock-step batches on a float handle
# ---------------------------------------------------------------------------------------------
def _fit_predict_alone(lib, H, spec, X, y, u0, Xs, T, lr):
    """gpimhip_fit_exact + gpimhip_predict_exact of one problem: (history, losses, final u, mean, var)"""
    m, P, N, M = spec.struct(), spec.n_params, len(X), len(Xs)
    Xd, yd, Xsd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (X, y, Xs))
    u = u0.clone().cuda()
    hist = torch.empty(T, P, dtype=torch.float64, device="cuda")
    loss = torch.empty(T, dtype=torch.float64, device="cuda")
    lib.check(H.lib.gpimhip_fit_exact(H.h, ctypes.byref(m), lib.ptr(Xd), lib.ptr(yd), N, lib.ptr(u), lr, T,
                                      lib.ptr(hist), lib.ptr(loss)))
    mean = torch.empty(M, dtype=torch.float64, device="cuda")
    var = torch.empty_like(mean)
    lib.check(H.lib.gpimhip_predict_exact(H.h, ctypes.byref(m), lib.ptr(Xd), lib.ptr(yd), N, lib.ptr(u), lib.ptr(Xsd), M,
                                          lib.ptr(mean), lib.ptr(var)))
    return tuple(t.cpu().numpy() for t in (hist, loss, u, mean, var))


# B = 3: the step launches host the tiles of all problems; B = 6: the `B > 4` branch (the fill as a tile-engine launch
# of its own, the factorisation role alone).  Hosted tiles per step launch times B, from gpimhip_step_plan_host_f32: at
# most 8 x 3 at N = 1207 and 27 x 4 = 108 at N = 2300 -- all quadrants; the whole-tile shape needs nf * B > 512, which a
# batch of four reaches from 36 block columns: N = 4500 (133 x 4, three launches; truth: the double handle).
@pytest.mark.parametrize("N,B", [(300, 3), (1207, 3), (2300, 4), (300, 6), (1207, 6), (4500, 4)])
def test_float_batch_equals_stand_alone_and_truth(lib, N, B):
    """gpimhip_fit_exact_batched (T = 4) + gpimhip_predict_exact_batched on a float handle, distinct X per problem:
    every problem bit-identical to its stand-alone fit + predict on a fresh float handle (the promise the double
    engine makes and tests: the same tile operations in the same k order whatever the launch shape), and held to the
    bars above against the truth -- the loss at the initial u and the posterior at the fitted u."""
    from problems import oracle_threads
    T, lr, kind = 4, 0.1, "Matern52"
    probs = [fixed_problem(N, 2, kind, seed=1000 * B + N + b) for b in range(B)]
    spec, u0, Xs = probs[0][3], probs[0][4], probs[0][5]
    m, P, M = spec.struct(), spec.n_params, len(Xs)
    Xd = torch.from_numpy(np.stack([p[0] for p in probs])).cuda().contiguous()
    yd = torch.from_numpy(np.stack([p[1] for p in probs])).cuda().contiguous()
    assert not np.array_equal(probs[0][0], probs[1][0])
    Xsd = torch.from_numpy(Xs).cuda()
    u = u0.repeat(B, 1).cuda().contiguous()
    hist = torch.empty(B, T, P, dtype=torch.float64, device="cuda")
    loss = torch.empty(B, T, dtype=torch.float64, device="cuda")
    mean = torch.empty(B, M, dtype=torch.float64, device="cuda")
    var = torch.empty_like(mean)
    H = lib.Handle(precision="single")
    try:
        lib.check(H.lib.gpimhip_fit_exact_batched(H.h, ctypes.byref(m), lib.ptr(Xd), N * 2, lib.ptr(yd), N, B, lib.ptr(u),
                                                  lr, T, lib.ptr(hist), lib.ptr(loss)))
        lib.check(H.lib.gpimhip_predict_exact_batched(H.h, ctypes.byref(m), lib.ptr(Xd), N * 2, lib.ptr(yd), N, B,
                                                      lib.ptr(u), lib.ptr(Xsd), M, lib.ptr(mean), lib.ptr(var)))
    finally:
        H.close()
    got = [t.cpu().numpy() for t in (hist, loss, u, mean, var)]
    for b, (X, y, kp, _, _, _) in enumerate(probs):
        Hs = lib.Handle(precision="single")
        try:
            want = _fit_predict_alone(lib, Hs, spec, X, y, u0, Xs, T, lr)
        finally:
            Hs.close()
        for name, g, w in zip(("history", "loss", "u", "mean", "var"), got, want):
            assert np.array_equal(g[b], w), "problem %d of %d: %s differs from the stand-alone run" % (b, B, name)
        ub = torch.from_numpy(got[2][b])
        if N <= 2300:
            with oracle_threads():
                loss_t = O.ExactGP(torch.from_numpy(X), torch.from_numpy(y), kp, JITTER).loss().item()
                with torch.no_grad():
                    kp.u_var.copy_(ub[0])
                    kp.u_ls.copy_(ub[1:1 + spec.n_ls])
                    kp.u_noise.copy_(ub[1 + spec.n_ls])
                mean_t, var_t = (t.numpy() for t in O.ExactGP(torch.from_numpy(X), torch.from_numpy(y), kp,
                                                              JITTER).predict(torch.from_numpy(Xs)))
        else:
            Hd = lib.Handle()
            try:
                loss_t = run_engine(lib, Hd, X, y, spec, u0, Xs)[0]
                _, _, mean_t, var_t = run_engine(lib, Hd, X, y, spec, ub, Xs)
            finally:
                Hd.close()
        print("N = %d, B = %d, problem %d: loss rel %.2e, mean %.2e, var %.2e" % (
            N, B, b, abs(got[1][b][0] - loss_t) / abs(loss_t), np.abs(got[3][b] - mean_t).max(),
            np.abs(got[4][b] - var_t).max()))
        assert_allclose(got[1][b][0], loss_t, rtol=5e-5)
        assert_allclose(got[3][b], mean_t, rtol=0, atol=2e-3 * (np.abs(mean_t).max() + 1))
        assert_allclose(got[4][b], var_t, rtol=2e-2, atol=1e-4)


# ---------------------------------------------------------------------------------------------
# prediction edges on a float handle
# ---------------------------------------------------------------------------------------------
def _predict(lib, H, spec, X, y, u, Xs):
    m, M = spec.struct(), len(Xs)
    Xd, yd, ud, Xsd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (X, y, u.numpy(), Xs))
    mean = torch.empty(M, dtype=torch.float64, device="cuda")
    var = torch.empty_like(mean)
    lib.check(H.lib.gpimhip_predict_exact(H.h, ctypes.byref(m), lib.ptr(Xd), lib.ptr(yd), len(X), lib.ptr(ud),
                                          lib.ptr(Xsd), M, lib.ptr(mean), lib.ptr(var)))
    return mean.cpu().numpy(), var.cpu().numpy()


def _posterior_bars(mean, var, mean_t, var_t):
    assert_allclose(mean, mean_t, rtol=0, atol=2e-3 * (np.abs(mean_t).max() + 1))
    assert_allclose(var, var_t, rtol=2e-2, atol=1e-4)


@pytest.fixture(scope="module")
def edge(lib):
    """N = 300 (three blocks, ragged last one), one float handle, the oracle's model"""
    X, y, kp, spec, u, Xs = fixed_problem(300, 2, "Matern52", seed=77)
    H = lib.Handle(precision="single")
    yield H, X, y, kp, spec, u, Xs
    H.close()


def _oracle_predict(kp, X, y, Xs):
    return tuple(t.numpy() for t in O.ExactGP(torch.from_numpy(X), torch.from_numpy(y), kp, JITTER).predict(
        torch.from_numpy(Xs)))


def test_edge_nan_row_and_single_point(lib, edge):
    H, X, y, kp, spec, u, Xs = edge
    mean0, var0 = _predict(lib, H, spec, X, y, u, Xs)
    mean_t, var_t = _oracle_predict(kp, X, y, Xs)
    _posterior_bars(mean0, var0, mean_t, var_t)
    Xn = Xs.copy()
    Xn[11, 1] = np.nan
    mean, var = _predict(lib, H, spec, X, y, u, Xn)
    assert np.isnan(mean[11]) and np.isnan(var[11])
    keep = np.arange(len(Xs)) != 11
    # the neighbours of the NaN row: what they are without it, bit for bit
    assert np.array_equal(mean[keep], mean0[keep]) and np.array_equal(var[keep], var0[keep])
    # M = 1
    mean1, var1 = _predict(lib, H, spec, X, y, u, Xs[7:8])
    assert mean1.shape == (1,)
    _posterior_bars(mean1, var1, mean_t[7:8], var_t[7:8])


def test_edge_several_slabs(lib, edge):
    """M = 4097: several slabs of test points, one point in the last."""
    H, X, y, kp, spec, u, _ = edge
    Xs = np.random.default_rng(5).uniform(0, X.max() + 1, size=(4097, 2))
    mean, var = _predict(lib, H, spec, X, y, u, Xs)
    _posterior_bars(mean, var, *_oracle_predict(kp, X, y, Xs))
    # a point's posterior does not depend on the slab it falls in
    m2, v2 = _predict(lib, H, spec, X, y, u, Xs[4000:])
    _posterior_bars(m2, v2, mean[4000:], var[4000:])
    assert np.abs(m2 - mean[4000:]).max() < 1e-6


@pytest.mark.parametrize("N", [384, 385])
def test_edge_predictor_switch_of_the_double_engine(lib, N, monkeypatch):
    """N = 384 / 385: a double handle switches between the fused predictor (which reads L^-1 in double) and the slab
    path here; a float handle takes the slab path at both -- the same bits with the fused predictor switched off."""
    X, y, kp, spec, u, Xs = fixed_problem(N, 2, "RBF", seed=N)
    out = []
    for knob in (None, "1"):
        if knob:
            monkeypatch.setenv("GPIMHIP_NO_FUSED_PREDICT", knob)
        else:
            monkeypatch.delenv("GPIMHIP_NO_FUSED_PREDICT", raising=False)
        H = lib.Handle(precision="single")
        try:
            out.append(_predict(lib, H, spec, X, y, u, Xs))
        finally:
            H.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    _posterior_bars(*out[0], *_oracle_predict(kp, X, y, Xs))


def test_edge_training_points_as_test_points(lib, edge):
    """At the training points k** - |L^-1 k*|^2 is a difference of nearly equal numbers (down to ~noise): whatever
    float32 makes of it, the clamp at zero keeps the variance at or above the noise, and finite."""
    H, X, y, kp, spec, u, _ = edge
    mean, var = _predict(lib, H, spec, X, y, u, X)
    noise = math.exp(U_NOISE)
    assert np.isfinite(mean).all() and np.isfinite(var).all()
    assert (var >= noise * (1 - 1e-6)).all()
    _posterior_bars(mean, var, *_oracle_predict(kp, X, y, X))


def test_edge_acquire_with_nan_mask(lib, edge):
    """gpimhip_acquire_exact with a mask holding NaN, float handle against double handle (the tolerances of
    test_acquire_exact_on_single_precision_handle)."""
    H32, X, y, kp, spec, u, _ = edge
    N = len(X)
    side = X.max() + 1
    g = np.stack(np.meshgrid(np.linspace(0, side, 40), np.linspace(0, side, 40), indexing="ij"), -1).reshape(-1, 2)
    M = len(g)
    mask = np.ones(M)
    mask[[0, 17, 800, M - 1]] = np.nan
    out = {}
    H64 = lib.Handle()
    try:
        for name, H in (("s", H32), ("d", H64)):
            Xd, yd, ud, gd, md = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (X, y, u.numpy(), g, mask))
            mean = torch.empty(M, dtype=torch.float64, device="cuda")
            sd, acq = torch.empty_like(mean), torch.empty_like(mean)
            m = spec.struct()
            lib.check(H.lib.gpimhip_acquire_exact(H.h, ctypes.byref(m), lib.ptr(Xd), lib.ptr(yd), N, lib.ptr(ud),
                                                  lib.ptr(gd), M, lib.ptr(Xd), N, lib.ACQ_IDS["ei"], 0.0, 0.01,
                                                  lib.ptr(md), lib.ptr(mean), lib.ptr(sd), lib.ptr(acq)))
            out[name] = (mean.cpu().numpy(), sd.cpu().numpy(), acq.cpu().numpy())
    finally:
        H64.close()
    nan = np.isnan(mask)
    for name in ("s", "d"):
        assert np.isnan(out[name][2][nan]).all() and np.isfinite(out[name][2][~nan]).all()
        assert np.isfinite(out[name][0]).all() and np.isfinite(out[name][1]).all()
    assert_allclose(out["s"][0], out["d"][0], rtol=0, atol=2e-4)
    assert_allclose(out["s"][1], out["d"][1], rtol=2e-3, atol=1e-5)
    assert_allclose(out["s"][2][~nan], out["d"][2][~nan], rtol=0, atol=2e-3 * (np.abs(out["d"][2][~nan]).max() + 1e-12))
