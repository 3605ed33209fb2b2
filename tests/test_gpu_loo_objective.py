"""
The leave-one-out objective on the MI355X: gpimhip_loo_grad / gpimhip_fit_exact_loo through the C ABI
against torch autograd (tests/loo_objective_oracle.py), workspace hygiene bit for bit, the tie to rec.loo() and the Python
surface.  fp64 throughout; the bars are those tests/test_gpu_ops.py holds gpimhip_nll_grad and gpimhip_fit_exact to.
"""
import ctypes
import math

import numpy as np
import pytest
import torch
from numpy.testing import assert_allclose

pytestmark = pytest.mark.gpu

import loo_objective_oracle as LG
import loo_oracle as LO
from oracle import gpim_oracle as O


@pytest.fixture(scope="module")
def eng(ensure_built):
    from gpim_amd import _lib
    H = _lib.Handle()
    yield _lib, H
    H.close()


def _grad_call(_lib, H, fn, spec, Xd, yd, ud):
    """(loss, gradient) host tensors of gpimhip_nll_grad / gpimhip_loo_grad (fn) -- the whole output buffer, for bit compares"""
    out = torch.empty(1 + spec.n_params, dtype=torch.float64, device="cuda")
    m = spec.struct()
    _lib.check(fn(H.h, ctypes.byref(m), _lib.ptr(Xd), _lib.ptr(yd), Xd.shape[0], _lib.ptr(ud),
                  ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(out.data_ptr() + 8)))
    return out.cpu()


def _device_problem(kind, N, d, iso):
    kp, spec, u, X, y = LO.problem(kind, N, d, iso)
    return kp, spec, X.cuda().contiguous(), y.cuda().contiguous(), u.cuda()


# ---------------------------------------------------------------------------------------------- 1. parity
# The spread of the two CPU references per case (tests/test_loo_objective_host.py prints it): loss relative, gradient
# absolute.  All are below a tenth of the bar (loss 1e-13; gradient 1e-11 + 1e-11 |g|), so every case keeps the bar of
# gpimhip_nll_grad.
#   RBF 7 d2            2.4e-16   6.2e-15        RationalQuadratic 200 d3   8.6e-15   4.3e-13
#   Matern52 40 d2      6.4e-15   1.1e-13        RBF 300 d2 isotropic       3.3e-15   3.4e-12  (|g| up to 116)
#   RBF 130 d3          2.0e-15   2.0e-13        Matern52 530 d3            1.7e-14   1.7e-12  (|g| up to 133)
#   Matern52 257 d4     1.1e-15   1.5e-13
@pytest.mark.parametrize("kind,N,d,iso", LG.CASES)
def test_loo_grad_matches_autograd(eng, kind, N, d, iso):
    _lib, H = eng
    _, spec, Xd, yd, ud = _device_problem(kind, N, d, iso)
    loss_ref, g_ref = LG.reference(kind, N, d, iso)
    o = _grad_call(_lib, H, H.lib.gpimhip_loo_grad, spec, Xd, yd, ud)
    print("loo_grad %s N=%d: loss rel %.2e, grad abs %.2e" % (kind, N, abs(o[0].item() / loss_ref - 1.0),
                                                                np.abs(o[1:].numpy() - g_ref).max()))
    assert_allclose(o[0].item(), loss_ref, rtol=1e-12)
    assert_allclose(o[1:].numpy(), g_ref, rtol=1e-10, atol=1e-10)


# ---------------------------------------------------------------------------------------------- 2. trajectory
def _trajectory_reference(kind):
    X, y = LO.scattered(60, 2, seed=3)
    torch.manual_seed(0)
    kp = O.KernelParams(kind, 2, [[0.5, 0.5], [12., 12.]])
    return (X, y) + LG.adam_path(kp, X, y, 0.05, 200, jitter=1e-6)


_trajectory_cache = {}


def trajectory_reference(kind):
    if kind not in _trajectory_cache:
        _trajectory_cache[kind] = _trajectory_reference(kind)
    return _trajectory_cache[kind]


@pytest.mark.parametrize("kind", ["RBF", "Matern52"])
def test_fit_trajectory_loo(eng, kind):
    """200 Adam iterations on the leave-one-out objective: the whole hyper-parameter history follows torch.optim.Adam on
    autograd's loss (test_fit_trajectory's setup and bars)."""
    _lib, H = eng
    X, y, ref, ref_loss = trajectory_reference(kind)
    from gpim_amd.kernels import KernelSpec
    torch.manual_seed(0)
    spec = KernelSpec(kind, 2, [[0.5, 0.5], [12., 12.]], jitter=1e-6)
    u = spec.draw_initial_u().cuda()
    m = spec.struct()
    Xd, yd = X.cuda().contiguous(), y.cuda().contiguous()
    hist = torch.empty(200, 4, dtype=torch.float64, device="cuda")
    loss = torch.empty(200, dtype=torch.float64, device="cuda")
    _lib.check(H.lib.gpimhip_fit_exact_loo(H.h, ctypes.byref(m), _lib.ptr(Xd), _lib.ptr(yd), len(X), _lib.ptr(u),
                                           0.05, 200, _lib.ptr(hist), _lib.ptr(loss)))
    print("trajectory %s: history rel %.2e, loss rel %.2e" % (kind, np.abs(hist.cpu().numpy() / ref - 1.0).max(),
                                                            np.abs(loss.cpu().numpy() / ref_loss - 1.0).max()))
    assert_allclose(hist.cpu().numpy(), ref, rtol=1e-8)
    assert_allclose(loss.cpu().numpy(), ref_loss, rtol=1e-10)


# ---------------------------------------------------------------------------------------------- 3. workspace hygiene
def test_two_calls_same_bits(eng):
    _lib, H = eng
    _, spec, Xd, yd, ud = _device_problem("Matern52", 530, 3, False)
    a = _grad_call(_lib, H, H.lib.gpimhip_loo_grad, spec, Xd, yd, ud)
    b = _grad_call(_lib, H, H.lib.gpimhip_loo_grad, spec, Xd, yd, ud)
    assert torch.equal(a, b) and torch.isfinite(a).all()


def test_used_handle_gives_fresh_handle_bits(ensure_built):
    """A handle that trained at N = 600 (five block rows, every padding row of the workspace matrices written: not ragged)
    gives at N = 530 (the same five block rows, ragged: 18 valid rows in the last) the bits of a fresh handle -- nothing
    reads stale padding, a stale temporary or a stale inverse."""
    from gpim_amd import _lib
    _, spec, Xd, yd, ud = _device_problem("Matern52", 530, 3, False)
    fresh, used = _lib.Handle(), _lib.Handle()
    try:
        want = _grad_call(_lib, fresh, fresh.lib.gpimhip_loo_grad, spec, Xd, yd, ud)
        _, spec6, X6, y6, u6 = _device_problem("Matern52", 600, 3, False)
        m6 = spec6.struct()
        hist = torch.empty(3, spec6.n_params, dtype=torch.float64, device="cuda")
        _lib.check(used.lib.gpimhip_fit_exact(used.h, ctypes.byref(m6), _lib.ptr(X6), _lib.ptr(y6), X6.shape[0],
                                              _lib.ptr(u6.clone()), 0.05, 3, _lib.ptr(hist), None))
        got = _grad_call(_lib, used, used.lib.gpimhip_loo_grad, spec, Xd, yd, ud)
        assert torch.equal(got, want)
    finally:
        fresh.close()
        used.close()


@pytest.mark.parametrize("N", [300, 530])
def test_nll_and_predict_unchanged_by_loo_calls(eng, N):
    """gpimhip_nll_grad and gpimhip_predict_exact give the same bits before and after gpimhip_loo_grad and
    gpimhip_fit_exact_loo on the same handle: the objective leaves G2 where S^-1 was, and nothing may take it for S^-1."""
    _lib, H = eng
    _, spec, Xd, yd, ud = _device_problem("Matern52", N, 3, False)
    m = spec.struct()
    Xs = torch.from_numpy(np.random.default_rng(5).uniform(0, 24, size=(200, 3))).cuda().contiguous()

    def state():
        g = _grad_call(_lib, H, H.lib.gpimhip_nll_grad, spec, Xd, yd, ud)
        mean = torch.empty(200, dtype=torch.float64, device="cuda")
        var = torch.empty_like(mean)
        _lib.check(H.lib.gpimhip_predict_exact(H.h, ctypes.byref(m), _lib.ptr(Xd), _lib.ptr(yd), N, _lib.ptr(ud), _lib.ptr(Xs),
                                               200, _lib.ptr(mean), _lib.ptr(var)))
        return g, mean.cpu(), var.cpu()

    before = state()
    _grad_call(_lib, H, H.lib.gpimhip_loo_grad, spec, Xd, yd, ud)
    mid = state()
    u2 = ud.clone()
    hist = torch.empty(9, spec.n_params, dtype=torch.float64, device="cuda")
    _lib.check(H.lib.gpimhip_fit_exact_loo(H.h, ctypes.byref(m), _lib.ptr(Xd), _lib.ptr(yd), N, _lib.ptr(u2), 0.05, 9,
                                           _lib.ptr(hist), None))
    after = state()
    for a, b, c in zip(before, mid, after):
        assert torch.equal(a, b) and torch.equal(a, c)


# ---------------------------------------------------------------------------------------------- 4. tie to rec.loo()
def _scattered_image(N, seed):
    """an image with N observed pixels (the rest NaN)"""
    rng = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(24.0), np.arange(24.0), indexing="ij")
    R = np.sin((ii + jj) / 5.0) + 0.1 * rng.standard_normal(ii.shape)
    R.ravel()[rng.permutation(R.size)[N:]] = np.nan
    return R


@pytest.mark.parametrize("N", [130, 300])
def test_loss_is_negated_elpd_of_rec_loo(ensure_built, N):
    """rec.loss_and_grad()[0] of an objective='loo' model = -sum_i log N(y_i | mean_i, var_i + jitter) + prior constant,
    recomputed in float64 from rec.loo(as_grid=False)'s arrays."""
    import gpim_amd
    R = _scattered_image(N, seed=N)
    X, Xf = gpim_amd.utils.get_sparse_grid(R), gpim_amd.utils.get_full_grid(R)
    rec = gpim_amd.reconstructor(X, R, Xf, kernel="Matern52", lengthscale=[[0.5, 0.5], [12., 12.]], verbose=0, objective="loo")
    rec._u[1 + rec._spec.n_ls] = -3.0
    loss, grad = rec.loss_and_grad()
    mean, sd, score = rec.loo(as_grid=False)
    assert score["n"] == N
    y = rec.y.numpy().astype(np.float64)
    var = sd.astype(np.float64) ** 2 + rec._spec.jitter
    assert (sd.astype(np.float64) ** 2 > math.exp(-3.0)).all()          # nothing clamped
    elpd = np.sum(-0.5 * (np.log(2.0 * math.pi * var) + (y - mean) ** 2 / var))
    spec = rec._spec
    prior = math.log(spec.amp_hi - spec.amp_lo) + sum(math.log(h - l) for l, h in zip(spec.ls_lo, spec.ls_hi))
    assert_allclose(loss, -elpd + prior, rtol=1e-10)
    assert torch.isfinite(grad).all()


# ---------------------------------------------------------------------------------------------- 5. surface
@pytest.mark.parametrize("kind", ["RBF", "Matern52"])
def test_reconstructor_trains_on_loo(ensure_built, kind):
    """reconstructor(objective='loo').train() reproduces the C-ABI trajectory's reference through Python."""
    import gpim_amd
    X, y, ref, ref_loss = trajectory_reference(kind)
    R = np.full((24, 24), np.nan)
    R[X[:, 0].long().numpy(), X[:, 1].long().numpy()] = y.numpy()
    Xs, Xf = gpim_amd.utils.get_sparse_grid(R), gpim_amd.utils.get_full_grid(R)
    rec = gpim_amd.reconstructor(Xs, R, Xf, kernel=kind, lengthscale=[[0.5, 0.5], [12., 12.]], learning_rate=0.05,
                                 iterations=200, verbose=0, seed=0, jitter=1e-6, objective="loo")
    assert rec.objective == "loo"
    assert len(rec.X) == len(X)
    rec.train()
    hist = np.column_stack([rec.hyperparams["variance"], np.array(rec.hyperparams["lengthscale"]), rec.hyperparams["noise"]])
    # (a permutation of the rows changes the summation order, not the model: the bars of the trajectory test hold)
    assert_allclose(hist, ref, rtol=1e-8)
    assert_allclose(np.array(rec.loss_all), ref_loss, rtol=1e-10)


def test_default_objective_is_nll(ensure_built):
    """objective='nll' and no keyword give identical histories -- and not the leave-one-out model's."""
    import gpim_amd
    R = _scattered_image(150, seed=2)
    X, Xf = gpim_amd.utils.get_sparse_grid(R), gpim_amd.utils.get_full_grid(R)
    runs = []
    for kw in ({}, {"objective": "nll"}, {"objective": "loo"}):
        rec = gpim_amd.reconstructor(X, R, Xf, kernel="RBF", learning_rate=0.1, iterations=12, verbose=0, **kw)
        rec.train()
        runs.append((rec.objective, rec.hyperparams["lengthscale"], rec.hyperparams["noise"], rec.loss_all))
    assert runs[0][0] == runs[1][0] == "nll" and runs[2][0] == "loo"
    assert runs[0][1:] == runs[1][1:]
    assert runs[0][3] != runs[2][3]


def test_boptimizer_forwards_objective(ensure_built):
    import gpim_amd
    rng = np.random.default_rng(0)
    ii, jj = np.meshgrid(np.arange(12.0), np.arange(12.0), indexing="ij")
    Z = np.exp(-((ii - 7) ** 2 + (jj - 4) ** 2) / 18.0)
    R = np.full_like(Z, np.nan)
    seed_idx = rng.permutation(Z.size)[:30]
    R.ravel()[seed_idx] = Z.ravel()[seed_idx]
    X, Xf = gpim_amd.utils.get_sparse_grid(R), gpim_amd.utils.get_full_grid(R)
    bo = gpim_amd.boptimizer(X, R, Xf, lambda idx: Z[tuple(idx)], acquisition_function="cb", exploration_steps=2,
                             gp_iterations=20, verbose=0, objective="loo", lengthscale=[[1., 1.], [8., 8.]])
    assert bo.surrogate_model.objective == "loo"
    bo.run()
    assert len(bo.indices_all) == 2 and len(bo.surrogate_model.loss_all) >= 40
    assert np.isfinite(bo.surrogate_model.loss_all).all()
    assert gpim_amd.boptimizer(X, R, Xf, lambda idx: Z[tuple(idx)], verbose=0).surrogate_model.objective == "nll"


def test_skreconstructor_forwards_objective(ensure_built):
    """An incomplete grid that skreconstructor hands to the dense solver trains on the objective; the structured solvers
    refuse it with their reason."""
    import gpim_amd
    R = _scattered_image(150, seed=4)
    X, Xf = gpim_amd.utils.get_sparse_grid(R), gpim_amd.utils.get_full_grid(R)
    rec = gpim_amd.skreconstructor(X, R, Xf, kernel="Matern52", iterations=5, verbose=0, objective="loo")
    assert rec.solver == "dense" and rec.objective == "loo"
    rec.train()
    assert len(rec.loss_all) == 5 and np.isfinite(rec.loss_all).all()
    Rf = np.cos(ii_jj(12, 12))
    Xg = gpim_amd.utils.get_full_grid(Rf)
    with pytest.raises(NotImplementedError, match="objective='loo'.*Reflection solver"):
        gpim_amd.skreconstructor(Xg, Rf, Xg, kernel="Matern52", objective="loo")


def ii_jj(n, m):
    ii, jj = np.meshgrid(np.arange(float(n)), np.arange(float(m)), indexing="ij")
    return ii / 3.0 + jj / 4.0


def test_python_refusals(ensure_built):
    import gpim_amd
    R = _scattered_image(100, seed=1)
    X, Xf = gpim_amd.utils.get_sparse_grid(R), gpim_amd.utils.get_full_grid(R)
    with pytest.raises(ValueError, match="objective must be 'nll' or 'loo'"):
        gpim_amd.reconstructor(X, R, Xf, objective="elpd")
    with pytest.raises(NotImplementedError, match="objective='loo'.*Sparse solver.*inducing points"):
        gpim_amd.reconstructor(X, R, Xf, sparse=True, indpoints=20, objective="loo")
    with pytest.raises(NotImplementedError, match="objective='loo'.*single precision"):
        gpim_amd.reconstructor(X, R, Xf, precision="single", objective="loo")
    Rf = np.cos(ii_jj(12, 12))
    Xg = gpim_amd.utils.get_full_grid(Rf)
    with pytest.raises(NotImplementedError, match="objective='loo'.*Kron solver"):
        gpim_amd.reconstructor(Xg, Rf, Xg, structured=True, objective="loo")
    with pytest.raises(NotImplementedError, match="objective='loo'.*Reflection solver"):
        gpim_amd.reconstructor(Xg, Rf, Xg, kernel="RationalQuadratic", structured=True, objective="loo")
    Rc = Rf.copy()
    Rc[3, :] = np.nan                                   # a whole row missing: the column-blocks solver
    with pytest.raises(NotImplementedError, match="objective='loo'.*(Columns|Reflection) solver"):
        gpim_amd.skreconstructor(gpim_amd.utils.get_sparse_grid(Rc), Rc, Xg, objective="loo")
    with pytest.raises(NotImplementedError, match="objective='loo'.*spectral-mixture"):
        gpim_amd.skreconstructor(Xg, Rf, Xg, kernel="Spectral", objective="loo")
    with pytest.raises(NotImplementedError, match="objective='loo'.*multi-output"):
        gpim_amd.vreconstructor(Xg, np.stack([Rf, -Rf], axis=-1), Xg, objective="loo")
    # a structured model built for the marginal likelihood: its solver refuses the calls themselves
    rec = gpim_amd.reconstructor(Xg, Rf, Xg, structured=True, verbose=0)
    rec.objective = "loo"
    with pytest.raises(NotImplementedError, match="objective='loo': the Kron solver"):
        rec.loss_and_grad()
    with pytest.raises(NotImplementedError, match="objective='loo': the Kron solver"):
        rec.train(iterations=2)


def test_c_entries_refuse_what_they_do_not_compute(ensure_built):
    """GPIMHIP_E_BADARG with a message: a single-precision handle, reflection mode."""
    from gpim_amd import _lib
    _, spec, Xd, yd, ud = _device_problem("RBF", 130, 3, False)
    m = spec.struct()
    out = torch.empty(1 + spec.n_params, dtype=torch.float64, device="cuda")
    hist = torch.empty(2, spec.n_params, dtype=torch.float64, device="cuda")

    def both(H):
        rc1 = H.lib.gpimhip_loo_grad(H.h, ctypes.byref(m), _lib.ptr(Xd), _lib.ptr(yd), 130, _lib.ptr(ud),
                                     ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(out.data_ptr() + 8))
        msg1 = H.lib.gpimhip_last_error().decode()
        rc2 = H.lib.gpimhip_fit_exact_loo(H.h, ctypes.byref(m), _lib.ptr(Xd), _lib.ptr(yd), 130, _lib.ptr(ud.clone()), 0.05, 2,
                                          _lib.ptr(hist), None)
        msg2 = H.lib.gpimhip_last_error().decode()
        return (rc1, msg1), (rc2, msg2)

    H32 = _lib.Handle(precision="single")
    try:
        for rc, msg in both(H32):
            assert rc == _lib.E_BADARG and "single-precision handle" in msg
    finally:
        H32.close()
    H = _lib.Handle()
    try:
        twoc = (ctypes.c_double * 4)(23.0, 23.0, 23.0, 0.0)
        _lib.check(H.lib.gpimhip_set_reflection(H.h, 1, twoc, None, 260, 0))
        for rc, msg in both(H):
            assert rc == _lib.E_BADARG and "reflection mode" in msg
        _lib.check(H.lib.gpimhip_set_reflection(H.h, 0, None, None, 0, 0))
        (rc, _), _ = both(H)
        assert rc == _lib.OK
    finally:
        H.close()
