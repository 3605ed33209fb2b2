"""
The fused trainer for N <= 128 (gpim_amd/csrc/smalln.hip: fit_small_kernel, the whole Adam loop in one workgroup around
lds_factor_inv of blocklds.hpp) against the CPU oracle (oracle/gpim_oracle.py: O.ExactGP, float64 autograd), size by size.

What the sizes pin (npan = ceil(N / 16) panels; the work plan of lds_factor_inv differs for every npan, and its host
replay is tests/test_fi_plan_host.py):

    N        1 2 15 16 | 17 31 32 | 33 47 48 | 49 64 | 65 80 | 81 96 | 97 112 | 113 127 128
    npan         1     |    2     |    3     |   4   |   5   |   6   |   7    |      8
    split        4     |    4     |    1 from N = 33 (more than three 16 x 16 tiles: one tile per wave and round)
    padding  16 k: none; 16 k + 1: fifteen identity rows; N = 1: the block is one observation and fifteen padding rows

Inputs: the `scattered` / `pair` problems of test_gpu_ops.py at noise_u = -3, jitter 1e-5, lengthscale bounds [0.5, 12] on
the 24-grid -- the conditioning the bars of test_kmat_nll_grad_predict / test_fit_trajectory are stated for.  (d = 1: the
24-grid has 24 distinct points, so one-dimensional problems draw from the integer grid 0 .. max(24, 4 N) - 1.)
Every case also runs through the general blocked path (GPIMHIP_NO_SMALLN=1) on the same inputs and is held to the same
bars: a case that passes there and fails here is a finding about smalln.hip / blocklds.hpp.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
from numpy.testing import assert_allclose

from oracle import gpim_oracle as O
from test_gpu_ops import pair, scattered

pytestmark = pytest.mark.gpu

PATHS = ["fused", "general"]


@pytest.fixture(scope="module")
def eng(ensure_built):
    from gpim_amd import _lib
    H = _lib.Handle()
    yield _lib, H
    H.close()


def use_path(monkeypatch, path):
    if path == "general":
        monkeypatch.setenv("GPIMHIP_NO_SMALLN", "1")
    else:
        monkeypatch.delenv("GPIMHIP_NO_SMALLN", raising=False)


def bounds(d, iso):
    return [0.5, 12.0] if iso else [[0.5] * d, [12.0] * d]


def points(N, d, seed):
    X, y = scattered(N, d, seed=seed, grid=24 if d > 1 else max(24, 4 * N))
    assert len(X) == N
    return X, y


# ---- the oracle's side: computed once per problem, never modified afterwards ---------------------------------------------
@functools.lru_cache(maxsize=None)
def nll_problem(kind, N, d, iso):
    """inputs, oracle loss and gradient with respect to u"""
    X, y = points(N, d, seed=7 * N + d)
    kp, spec, u = pair(kind, d, bounds(d, iso), seed=N)
    loss, g = O.ExactGP(X, y, kp, 1e-5).loss_and_grad()
    return X, y, spec, u, loss.item(), g.numpy().copy()


def oracle_adam(X, y, kp, jitter, lr, T):
    """torch.optim.Adam on the oracle's loss: (history rows [variance, lengthscale.., noise(, alpha)], losses, completed
    iterations -- fewer than T when torch.linalg.cholesky raises)"""
    gp = O.ExactGP(X, y, kp, jitter)
    opt = torch.optim.Adam(kp.parameters(), lr=lr)
    hist, losses = [], []
    for _ in range(T):
        opt.zero_grad()
        try:
            loss = gp.loss()
        except torch.linalg.LinAlgError:
            break
        loss.backward()
        opt.step()
        losses.append(loss.item())
        row = [kp.variance.item(), *kp.lengthscale.reshape(-1).tolist(), kp.noise.item()]
        if kp.kind == "RationalQuadratic":
            row.append(kp.scale_mixture.item())
        hist.append(row)
    return np.array(hist), np.array(losses), len(losses)


T_FIT, LR_FIT = 40, 0.05


@functools.lru_cache(maxsize=None)
def fit_problem(kind, N, d, iso, xseed, useed, yshift=0):
    """inputs and the oracle's 40-iteration trajectory; yshift != 0: another target on the same X"""
    X, y = points(N, d, seed=xseed)
    if yshift:
        y = y + torch.cos(X.sum(1) / (3.0 + yshift)) * 0.5
    kp, spec, u = pair(kind, d, bounds(d, iso), seed=useed)
    hist, losses, done = oracle_adam(X, y, kp, 1e-5, LR_FIT, T_FIT)
    assert done == T_FIT
    return X, y, spec, u, hist, losses


# ---- the engine's side --------------------------------------------------------------------------------------------------
def nll_grad(_lib, H, spec, X, y, u):
    m = spec.struct()
    Xd, yd, ud = X.cuda().contiguous(), y.cuda().contiguous(), u.cuda()
    out = torch.full((1 + spec.n_params,), float("nan"), dtype=torch.float64, device="cuda")
    rc = H.lib.gpimhip_nll_grad(H.h, ctypes.byref(m), _lib.ptr(Xd), _lib.ptr(yd), len(X), _lib.ptr(ud),
                                ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(out.data_ptr() + 8))
    return rc, out.cpu().numpy()


def fit_one(_lib, H, spec, X, y, u, lr, T):
    """gpimhip_fit_exact: (rc, history T x P, losses T, final u); rows the engine did not write stay NaN"""
    m = spec.struct()
    Xd, yd, ud = X.cuda().contiguous(), y.cuda().contiguous(), u.clone().cuda()
    hist = torch.full((T, spec.n_params), float("nan"), dtype=torch.float64, device="cuda")
    loss = torch.full((T,), float("nan"), dtype=torch.float64, device="cuda")
    rc = H.lib.gpimhip_fit_exact(H.h, ctypes.byref(m), _lib.ptr(Xd), _lib.ptr(yd), len(X), _lib.ptr(ud), lr, T,
                                 _lib.ptr(hist), _lib.ptr(loss))
    return rc, hist.cpu(), loss.cpu(), ud.cpu()


def fit_batch(_lib, H, spec, Xs, ys, us, lr, T):
    """gpimhip_fit_exact_batched; Xs: one (N, d) tensor (shared, x_stride 0) or a list of B of them"""
    m = spec.struct()
    shared = not isinstance(Xs, (list, tuple))
    N = len(Xs) if shared else len(Xs[0])
    B = len(ys)
    Xd = (Xs if shared else torch.stack(list(Xs))).cuda().contiguous()
    yd, ud = torch.stack(list(ys)).cuda().contiguous(), torch.stack(list(us)).cuda().contiguous()
    hist = torch.full((B, T, spec.n_params), float("nan"), dtype=torch.float64, device="cuda")
    loss = torch.full((B, T), float("nan"), dtype=torch.float64, device="cuda")
    rc = H.lib.gpimhip_fit_exact_batched(H.h, ctypes.byref(m), _lib.ptr(Xd), 0 if shared else N * spec.dim, _lib.ptr(yd),
                                         N, B, _lib.ptr(ud), lr, T, _lib.ptr(hist), _lib.ptr(loss))
    return rc, hist.cpu(), loss.cpu(), ud.cpu()


def grad_err(g, g_ref):
    """the gradient's error on the scale of its bar (rtol = atol): max |g - g_ref| / (1 + |g_ref|)"""
    return float(np.max(np.abs(g - g_ref) / (1.0 + np.abs(g_ref))))


def assert_nll_bars(out, loss_ref, g_ref, tag):
    """the bars of test_kmat_nll_grad_predict; the figures are printed before they are asserted"""
    print("%s: loss rel. err %.2e (bar 1e-12), gradient err / (1 + |g|) %.2e (bar 1e-10)" % (
        tag, abs(out[0] - loss_ref) / abs(loss_ref), grad_err(out[1:], g_ref)))
    assert_allclose(out[0], loss_ref, rtol=1e-12)
    assert_allclose(out[1:], g_ref, rtol=1e-10, atol=1e-10)


def assert_fit_bars(hist, loss, hist_ref, loss_ref, tag):
    """the bars of test_fit_trajectory"""
    hist, loss = np.asarray(hist), np.asarray(loss)
    print("%s: history rel. err %.2e (bar 1e-8), loss rel. err %.2e (bar 1e-10)" % (
        tag, np.max(np.abs(hist / hist_ref - 1.0)), np.max(np.abs(loss / loss_ref - 1.0))))
    assert_allclose(hist, hist_ref, rtol=1e-8)
    assert_allclose(loss, loss_ref, rtol=1e-10)


# ---- (a) one evaluation of the loss and its gradient: gpimhip_nll_grad, the T == 0 path of fit_small_kernel ----------------
# (kind, N, d, isotropic): every N of the table above; RBF, Matern52 and RationalQuadratic each meet every npan; d = 1, 2, 3,
# 4 and the isotropic model each appear for N <= 32 and for N > 64
NLL_CASES = [
    # npan 1
    ("RBF", 1, 1, False), ("Matern52", 2, 2, False), ("RationalQuadratic", 15, 3, False), ("RBF", 16, 4, False),
    ("Matern52", 16, 2, True),
    # npan 2 (still four waves per tile)
    ("RationalQuadratic", 17, 1, False), ("RBF", 31, 2, True), ("Matern52", 32, 3, False),
    # npan 3 (one tile per wave and round from here)
    ("RationalQuadratic", 33, 4, False), ("RBF", 47, 3, False), ("Matern52", 48, 2, False),
    # npan 4
    ("RBF", 49, 2, False), ("Matern52", 49, 4, False), ("RationalQuadratic", 64, 2, True),
    # npan 5
    ("Matern52", 65, 1, False), ("RationalQuadratic", 65, 3, False), ("RBF", 80, 3, True),
    # npan 6
    ("RationalQuadratic", 81, 2, False), ("RBF", 96, 4, False), ("Matern52", 96, 3, False),
    # npan 7
    ("RBF", 97, 1, False), ("Matern52", 97, 2, True), ("RationalQuadratic", 112, 4, False),
    # npan 8
    ("Matern52", 113, 3, False), ("RationalQuadratic", 127, 2, False), ("RBF", 128, 2, False),
    ("Matern52", 128, 4, True), ("RationalQuadratic", 128, 1, False),
]


def test_nll_cases_cover_every_regime():
    """the written-out list above does what its comment says"""
    sizes = {1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 127, 128}
    assert {c[1] for c in NLL_CASES} == sizes
    for npan in range(1, 9):
        assert {c[0] for c in NLL_CASES if (c[1] + 15) // 16 == npan} == {"RBF", "Matern52", "RationalQuadratic"}
    for lo, hi in ((1, 32), (65, 128)):
        part = [c for c in NLL_CASES if lo <= c[1] <= hi]
        assert {c[2] for c in part if not c[3]} == {1, 2, 3, 4} and any(c[3] for c in part)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("kind,N,d,iso", NLL_CASES)
def test_nll_grad_every_size(eng, kind, N, d, iso, path, monkeypatch):
    _lib, H = eng
    use_path(monkeypatch, path)
    X, y, spec, u, loss_ref, g_ref = nll_problem(kind, N, d, iso)
    rc, out = nll_grad(_lib, H, spec, X, y, u)
    _lib.check(rc)
    assert_nll_bars(out, loss_ref, g_ref, "nll_grad %s N=%d d=%d iso=%d %s" % (kind, N, d, iso, path))


# ---- (b) trajectories: gpimhip_fit_exact, 40 Adam iterations at lr = 0.05 ---------------------------------------------------
FIT_CASES = [("RBF", 16, 2, False), ("Matern52", 17, 2, False), ("RationalQuadratic", 32, 2, False), ("RBF", 33, 3, False),
             ("Matern52", 80, 2, True), ("RationalQuadratic", 96, 3, False), ("RBF", 128, 2, False)]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("kind,N,d,iso", FIT_CASES)
def test_fit_trajectory_every_regime(eng, kind, N, d, iso, path, monkeypatch):
    """The whole history and the loss row follow the oracle's torch.optim.Adam loop at the bars of test_fit_trajectory
    (set for 200 iterations at N = 60)."""
    _lib, H = eng
    use_path(monkeypatch, path)
    X, y, spec, u, hist_ref, loss_ref = fit_problem(kind, N, d, iso, xseed=11 * N + d, useed=N)
    rc, hist, loss, _ = fit_one(_lib, H, spec, X, y, u, LR_FIT, T_FIT)
    _lib.check(rc)
    assert H.lib.gpimhip_fit_completed(H.h) == T_FIT
    assert_fit_bars(hist, loss, hist_ref, loss_ref, "fit %s N=%d d=%d iso=%d %s" % (kind, N, d, iso, path))


# ---- (c) batches: gpimhip_fit_exact_batched, one workgroup per problem ------------------------------------------------------
# (gpimhip_nll_grad_batched evaluates the coupled reflection blocks on the general path only: nothing of it runs here)
@pytest.mark.parametrize("shared_x", [False, True])
@pytest.mark.parametrize("kind,N,d,iso", [("Matern52", 33, 2, False), ("RationalQuadratic", 97, 3, False)])
def test_batch_is_five_single_fits(eng, kind, N, d, iso, shared_x):
    """B = 5 problems with their own X (x_stride = N d) or one shared X (x_stride = 0), five y and five u: the workgroups
    of the fused launch differ only in the pointer offsets taken from blockIdx.x, so every problem's history, losses and
    final u carry the bits of that problem run alone through gpimhip_fit_exact on a fresh handle; problems 0 and 4 also
    follow the oracle."""
    _lib, H = eng
    B = 5
    probs = [fit_problem(kind, N, d, iso, xseed=(13 * N + d) if shared_x else (13 * N + d + 100 * b), useed=N + b,
                         yshift=b if shared_x else 0) for b in range(B)]
    spec = probs[0][2]
    if shared_x:
        assert all(torch.equal(p[0], probs[0][0]) for p in probs) and not torch.equal(probs[0][1], probs[4][1])
    rc, hist, loss, u_end = fit_batch(_lib, H, spec, probs[0][0] if shared_x else [p[0] for p in probs],
                                      [p[1] for p in probs], [p[3] for p in probs], LR_FIT, T_FIT)
    _lib.check(rc)
    for b, (X, y, _, u, hist_ref, loss_ref) in enumerate(probs):
        H1 = _lib.Handle()
        try:
            rc1, h1, l1, u1 = fit_one(_lib, H1, spec, X, y, u, LR_FIT, T_FIT)
        finally:
            H1.close()
        _lib.check(rc1)
        assert torch.equal(hist[b], h1) and torch.equal(loss[b], l1) and torch.equal(u_end[b], u1), b
        if b in (0, 4):
            assert_fit_bars(hist[b], loss[b], hist_ref, loss_ref, "batch %s N=%d shared=%d problem %d" % (kind, N, shared_x, b))


# One problem of a batch turns not positive-definite at iteration k > 0: the construction of
# test_gpu_regimes.py::test_not_pd_freezes_at_failing_iteration (every point twice with identical targets, zero jitter,
# lr = 1: Adam lowers the noise by a factor e per iteration until K stops being numerically positive-definite) for problem 1;
# problems 0 and 2 are scattered points with noisy targets, which keep their noise.
MIX_N, MIX_T, MIX_LR, MIX_BAD = 50, 80, 1.0, 1


@functools.lru_cache(maxsize=None)
def mixed_batch():
    from gpim_amd.kernels import KernelSpec
    ls = [[1.0, 1.0], [10.0, 10.0]]
    ii, jj = np.meshgrid(np.arange(5.0), np.arange(5.0), indexing="ij")
    Xg = np.stack([ii.ravel(), jj.ravel()], 1)
    yg = np.sin(Xg[:, 0] / 3.0) * np.cos(Xg[:, 1] / 4.0)
    Xs, ys = [], []
    for b in range(3):
        if b == MIX_BAD:
            Xs.append(torch.from_numpy(np.concatenate([Xg, Xg])))
            ys.append(torch.from_numpy(np.concatenate([yg, yg])))
        else:
            X, y = points(MIX_N, 2, seed=500 + b)
            Xs.append(X)
            ys.append(y)
    torch.manual_seed(0)
    spec = KernelSpec("RBF", 2, ls, jitter=0.0)
    u0 = spec.draw_initial_u()
    refs = []
    for b in range(3):
        torch.manual_seed(0)
        refs.append(oracle_adam(Xs[b], ys[b], O.KernelParams("RBF", 2, ls), 0.0, MIX_LR, MIX_T))
    return spec, Xs, ys, u0, refs


def test_mixed_batch_one_problem_turns_not_pd(eng, monkeypatch):
    """gpimhip_fit_completed reports the failing iteration k, and the rows before it are the same on both paths.

    What the paths do with the healthy problems from row k on differs: the fused kernel's other workgroups run on -- a
    healthy problem's history, losses and final u are those of that problem fitted alone for all T iterations (asserted:
    same bits) -- while the lock-step path freezes the whole batch at iteration k: no row from k on is written for any
    problem and every u stays where iteration k - 1 left it.  The C ABI promises the common part (include/gpimhip.h:
    "u_inout and the first gpimhip_fit_completed() rows of hist_out / loss_out are valid after the error"), and
    gpim_amd/batch.py promises less: fit_predict_batch raises on GPIMHIP_E_NOT_PD before it returns anything, so no caller
    of it sees the rows or the parameters of either path.  Nothing a caller can observe through batch.py differs.

    Bars: rows before min(k_fused, k_general) at the bars of test_fit_trajectory for the healthy problems.  The failing
    problem runs towards a singular K: its gradient carries a relative error of cond(K) eps, and cond(K) grows by e per
    iteration up to 1 / eps at the failure, so two backward-stable evaluations agree to about e^-(k - i) at row i.  It is
    compared as test_not_pd_freezes_at_failing_iteration compares it -- rows before k - 10 at rtol 1e-4, the failing
    iterations of the two paths and of the oracle within 8 of each other -- and at the bars of test_fit_trajectory where
    that estimate is below them with a factor 100 to spare: rows before k - 23 (e^-23 = 1e-10).
    Measured: failing iteration 32 (fused), 33 (general), 37 (oracle); failing problem, fused against general, 1.8e-13
    before row k - 23 and 4.0e-8 before row k - 10; healthy problems 3.9e-12 (history) and 3.2e-11 (loss) over 32 rows."""
    _lib, H = eng
    spec, Xs, ys, u0, refs = mixed_batch()
    for b in range(3):
        assert (refs[b][2] < MIX_T) == (b == MIX_BAD)          # the oracle: exactly one problem fails
    k_ref = refs[MIX_BAD][2]
    res = {}
    for path in PATHS:
        use_path(monkeypatch, path)
        rc, hist, loss, u_end = fit_batch(_lib, H, spec, Xs, ys, [u0] * 3, MIX_LR, MIX_T)
        assert rc == _lib.E_NOT_PD
        res[path] = (H.lib.gpimhip_fit_completed(H.h), hist, loss, u_end)
        assert torch.isfinite(u_end).all()
    kf, kg = res["fused"][0], res["general"][0]
    print("failing iteration: fused %d, general %d, oracle %d" % (kf, kg, k_ref))
    assert 0 < kf < MIX_T and 0 < kg < MIX_T
    assert abs(kf - k_ref) <= 8 and abs(kg - k_ref) <= 8 and abs(kf - kg) <= 8
    k = min(kf, kg)
    for b in range(3):
        hf, lf = res["fused"][1][b].numpy(), res["fused"][2][b].numpy()
        hg, lg = res["general"][1][b].numpy(), res["general"][2][b].numpy()
        # the lock-step path: frozen at kg, every problem
        assert np.isfinite(hg[:kg]).all() and np.isnan(hg[kg:]).all() and np.isnan(lg[kg:]).all()
        if b == MIX_BAD:
            assert np.isfinite(hf[:kf]).all() and np.isnan(hf[kf:]).all() and np.isnan(lf[kf:]).all()
            kk = min(k, k_ref)
            assert kk > 23
            print("failing problem: history rel. diff fused / general %.2e before row %d, %.2e before row %d" % (
                np.max(np.abs(hf[:kk - 23] / hg[:kk - 23] - 1.0)), kk - 23, np.max(np.abs(hf[:kk - 10] / hg[:kk - 10] - 1.0)), kk - 10))
            assert_allclose(hf[:kk - 10], hg[:kk - 10], rtol=1e-4)
            assert_allclose(hf[:kk - 10], refs[b][0][:kk - 10], rtol=1e-4)
            assert_allclose(hf[:kk - 23], hg[:kk - 23], rtol=1e-8)
            assert_allclose(lf[:kk - 23], lg[:kk - 23], rtol=1e-10)
        else:
            print("healthy problem %d: history rel. diff fused / general %.2e, loss %.2e over %d rows" % (
                b, np.max(np.abs(hf[:k] / hg[:k] - 1.0)), np.max(np.abs(lf[:k] / lg[:k] - 1.0)), k))
            assert_allclose(hf[:k], hg[:k], rtol=1e-8)
            assert_allclose(lf[:k], lg[:k], rtol=1e-10)
            # the fused path: this workgroup ran on, exactly as if it were alone
            use_path(monkeypatch, "fused")
            H1 = _lib.Handle()
            try:
                rc1, h1, l1, u1 = fit_one(_lib, H1, spec, Xs[b], ys[b], u0, MIX_LR, MIX_T)
            finally:
                H1.close()
            _lib.check(rc1)
            assert torch.equal(res["fused"][1][b], h1) and torch.equal(res["fused"][2][b], l1)
            assert torch.equal(res["fused"][3][b], u1)


# ---- (d) not positive-definite, panel by panel --------------------------------------------------------------------------------
# The construction of test_gpu_ops.py::test_fit_reports_not_pd -- a duplicated point, noise_u = -800 (noise = 0) -- with
# row `pos` a copy of row pos // 2, pos at the first (for panel 0: the second), a middle and the last row of every panel.
#
# With ZERO jitter that K is exactly singular and the pivot of row pos is rounding noise of either sign, +- eps |K|: whether
# a factorisation fails there depends on its summation order.  Measured with zero jitter on 35 such positions at which
# torch.linalg.cholesky_ex failed on the oracle's K on one host: on a second host LAPACK passed 2 of them, and the engine
# returned 0 at 9 of them -- the fused and the general path at the same 9, both with a pivot just above zero, as LAPACK has
# at the positions it passes.  No return code can be asserted for such a matrix.  The jitter is therefore -1e-6 instead of
# 0: the 2 x 2 minor of the two copies is [[v - j, v], [v, v - j]], the pivot of row pos is -2 j = -2e-6 in exact
# arithmetic -- eight orders above the rounding noise of 1e-14 -- and every earlier pivot is above 0.4 (the oracle's K
# without the copy has its smallest eigenvalue at 0.089 for N = 128 and 1.7 for N = 50; checked on the CPU when this was
# written and again by the test through cholesky_ex).  Every reference and both paths must fail at exactly that row, so all
# positions of all panels stay and the failing column is asserted, not only the return code.
NOT_PD_JITTER = -1e-6


def not_pd_rows(N, q):
    lo, hi = 16 * q, min(16 * q + 15, N - 1)
    return sorted({max(lo, 1), min(lo + 8, hi), hi})


@functools.lru_cache(maxsize=None)
def not_pd_problem(N, pos):
    from gpim_amd.kernels import KernelSpec
    X, y = points(N, 2, seed=900 + N)
    X = X.clone()
    X[pos] = X[pos // 2]
    ls = [[0.5, 0.5], [2.0, 2.0]]
    torch.manual_seed(0)
    kp = O.KernelParams("RBF", 2, ls)
    torch.manual_seed(0)
    spec = KernelSpec("RBF", 2, ls, jitter=NOT_PD_JITTER)
    u = spec.draw_initial_u()
    u[3] = -800.0
    with torch.no_grad():
        kp.u_noise.fill_(-800.0)
        K = kp.K(X) + (NOT_PD_JITTER + kp.noise) * torch.eye(N, dtype=torch.float64)
    return X, y, spec, u, int(torch.linalg.cholesky_ex(K).info)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("N,q", [(N, q) for N in (128, 50) for q in range((N + 15) // 16)])
def test_not_pd_in_every_panel(eng, N, q, path, monkeypatch):
    """GPIMHIP_E_NOT_PD with the failing column, wherever the bad pivot falls, from both paths; and nothing of it sticks
    (s_bad / info): the next call on the same handle, a healthy problem of the same N, meets the bars of
    test_nll_grad_every_size."""
    import re
    _lib, H = eng
    use_path(monkeypatch, path)
    healthy = nll_problem("RBF", N, 2, False)
    rows = not_pd_rows(N, q)
    assert 2 <= len(rows) <= 3
    for pos in rows:
        assert pos // 16 == q and 0 < pos < N
        X, y, spec, u, info_ref = not_pd_problem(N, pos)
        assert info_ref == pos + 1                              # the reference fails at that row
        rc, _ = nll_grad(_lib, H, spec, X, y, u)
        assert rc == _lib.E_NOT_PD, (N, pos)
        msg = H.lib.gpimhip_last_error().decode()
        assert int(re.search(r"leading minor of order (\d+)", msg).group(1)) == pos + 1, msg
        X, y, spec, u, loss_ref, g_ref = healthy
        rc, out = nll_grad(_lib, H, spec, X, y, u)
        _lib.check(rc)
        assert_nll_bars(out, loss_ref, g_ref, "after not-PD at row %d: N=%d %s" % (pos, N, path))
