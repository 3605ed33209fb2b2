"""
Posterior draws of the dense-by-Kronecker blocks on the MI355X: skreconstructor.sample(method=
'columns') / gpimhip_sample_pkron against the dense numpy oracle of tests/columns_sample_oracle.py.

A draw is ``mean + A z``; the roots of the prior fix A only up to an orthogonal change of zeta, so the device is held to the
oracle through the covariance: one call with z = I (S = U_s U + N + M) returns A, and A A^T must be the rule's covariance
Sigma_post + c_n I + d T (I (x) K_c(u, u)) T^T.  Bar: 1e-9 max(1, s2), the bar of tests/test_gpu_kron_sample.py (the numpy
restatement of the identity leaves three orders of magnitude under it).  Hyper-parameters are fixed by writing u;
lengthscale bounds [[0.1] * d, [100] * d].
"""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import columns_sample_oracle as CO
from columns_oracle import cube

# the cubes of tests/test_gpu_columns.py, and a small one for the off-grid cases
CUBES = {
    "12x12x6": ((12, 12, 6), (0, 1), 0.4, 2),          # N_s = 86: one block column; U_s = 144, S = 2244
    "16x16x5": ((16, 16, 5), (0, 1), 0.35, 3),         # N_s = 166: two block columns, a ragged last one; prior factor of order 256
    "6x5x4x3": ((6, 5, 4, 3), (0, 1), 0.4, 1),         # two complete axes
    "5x12x12": ((5, 12, 12), (1, 2), 0.4, 4),          # spectral axis first: through the permutation
    "6x5x4": ((6, 5, 4), (0, 1), 0.6, 5),              # 12 pixels
}
# (cube, test grid): None its own; "half" the half-step grid (union axis != training axis: the second decomposition);
# "shift" shifted by 0.25 in every axis (no coincident rows: U_s = N_s + M_s)
CASES = [("12x12x6", None), ("16x16x5", None), ("6x5x4x3", None), ("5x12x12", None), ("6x5x4", "half"), ("6x5x4", "shift")]
_made, _recs = {}, {}


def data(name):
    if name not in _made:
        shape, cols, frac, seed = CUBES[name]
        _made[name] = cube(shape, cols, frac, seed=seed)
    return _made[name]


def axes_of(name, grid):
    shape = CUBES[name][0]
    if grid == "half":
        return [np.arange(0, n - 0.75, 0.5) for n in shape]
    if grid == "shift":
        return [np.arange(n, dtype=np.float64) + 0.25 for n in shape]
    return [np.arange(n, dtype=np.float64) for n in shape]


def grid_of(axes):
    return np.array(np.meshgrid(*axes, indexing="ij"))


def set_params(rec, ls, s2, noise):
    """writes u so that the constrained values are (s2, ls, noise) to rounding; returns the values the engine holds"""
    sp = rec._spec
    p = torch.cat([torch.tensor([(s2 - sp.amp_lo) / (sp.amp_hi - sp.amp_lo)], dtype=torch.float64),
                   (torch.tensor(ls, dtype=torch.float64) - sp.ls_lo) / (sp.ls_hi - sp.ls_lo)])
    u = torch.cat([torch.logit(p), torch.tensor([math.log(noise)], dtype=torch.float64)])
    rec._u[:u.numel()].copy_(u.to(rec._u.device))
    var, lsc, nz = sp.constrained(rec._u)
    return lsc.tolist(), float(var), float(nz)


def build(name, k, cls=None, **kw):
    """the model of cube `name` at parameter set k (cached), its engine-side parameters"""
    import gpim_amd
    key = (name, k, cls, tuple(sorted(kw.items())))
    if key not in _recs:
        Xg, X, R = data(name)
        d = len(CUBES[name][0])
        rec = (cls or gpim_amd.skreconstructor)(X, R, Xg, kernel="RBF", lengthscale=[[0.1] * d, [100.0] * d], verbose=0, **kw)
        s2, ls_r, lc, noise = CO.PARAMS[k]
        ls = [lc] * d
        for a, l in zip(CUBES[name][1], ls_r):            # the pixel axes are the ragged ones
            ls[a] = l
        _recs[key] = (rec, set_params(rec, ls, s2, noise))
    return _recs[key]


def oracle(rec, params, taxes, noiseless, jitter=CO.D):
    """the oracle's (A A^T's target, extra, Sigma_post, mean) in the test grid's own order, and the widths"""
    from gpim_amd import gprutils
    ls_e, s2_e, noise_e = params
    C = rec._solver.C
    rows, caxes, _, _ = rec._solver.sample_geometry(taxes)
    A, mean, cov, extra = CO.rule(C["Xs"], C["axes_c"], C["Y"], rows, caxes, s2_e, [ls_e[i] for i in C["ragged"]],
                                  [ls_e[i] for i in C["complete"]], noise_e, rec._spec.jitter, jitter, noiseless)
    o_idx = gprutils.column_sample_maps(C, [len(t) for t in taxes])[2]
    back = lambda Mx: Mx[o_idx][:, o_idx]
    return A[o_idx], mean[o_idx], back(cov), back(extra), CO.widths(C["Xs"], C["axes_c"], rows, caxes)


def draw_matrix(rec, taxes, W, noiseless, jitter=CO.D):
    """A of the device, (M, W), from one call with z = I, and predict's mean (M,)"""
    Xt = grid_of(taxes)
    out = rec.sample(n_samples=W, Xtest=Xt, z=np.eye(W), noiseless=noiseless, jitter=jitter, method="columns")
    assert out.shape == (W,) + Xt.shape[1:]
    mean = rec.predict(Xt)[0].reshape(-1)
    return (out.reshape(W, -1) - mean).T, mean


@pytest.mark.parametrize("k", (0, 1))
@pytest.mark.parametrize("name,grid", CASES, ids=["%s-%s" % (n, g or "own") for n, g in CASES])
def test_distribution_is_the_rule(name, grid, k):
    rec, params = build(name, k)
    assert rec.solver == "columns"
    taxes = axes_of(name, grid)
    bar = 1e-9 * max(1.0, CO.PARAMS[k][0])
    for noiseless in (False, True):
        _, mean_o, cov, extra, (Us, U, N, M) = oracle(rec, params, taxes, noiseless)
        W = Us * U + N + M
        if grid == "shift":
            assert Us == rec._solver.C["Xs"].shape[0] + M // int(np.prod([len(taxes[i]) for i in rec._solver.C["complete"]]))
        A, mean = draw_matrix(rec, taxes, W, noiseless)
        cn = 0.0 if noiseless else params[2]
        err = np.abs(A @ A.T - (cov + cn * np.eye(M) + extra)).max()
        print("%s/%s/%d noiseless=%d U_s=%d U=%d S=W=%d: max|A A^T - rule covariance| = %.3e (bar %.1e), max|extra| = %.3e, "
              "mean - oracle %.3e" % (name, grid or "own", k, noiseless, Us, U, W, err, bar, np.abs(extra).max(),
                                      np.abs(mean - mean_o).max()))
        assert np.isfinite(A).all()
        assert err <= bar
        assert np.abs(mean - mean_o).max() <= 1e-9


@pytest.mark.parametrize("name,grid", [("16x16x5", None), ("5x12x12", None), ("6x5x4", "half")],
                         ids=["16x16x5", "5x12x12", "6x5x4-half"])
def test_mean_bits_rows_and_grouping(name, grid):
    rec, params = build(name, 0)
    taxes = axes_of(name, grid)
    Xt = grid_of(taxes)
    Us, U, N, M = oracle(rec, params, taxes, False)[4]
    W = Us * U + N + M
    mean0, sd0 = rec.predict(Xt)
    # z = 0: predict's mean, bit for bit (the draws' update has no share of Y: section 23)
    out = rec.sample(n_samples=2, Xtest=Xt, z=np.zeros((2, W)), method="columns")
    assert out.shape == (2,) + Xt.shape[1:]
    assert np.array_equal(out[0], mean0) and np.array_equal(out[1], mean0)
    # mean_out of the entry point has predict's bits too
    sol = rec._solver
    zd = torch.zeros((1, W), dtype=torch.float64, device=rec._dev)
    mean_d = torch.empty(M, dtype=torch.float64, device=rec._dev)
    out_d = torch.empty((1, M), dtype=torch.float64, device=rec._dev)
    from gpim_amd import _lib
    _lib.check(sol.sample_columns(rec, taxes, zd, False, CO.D, mean_d, out_d))
    assert np.array_equal(mean_d.cpu().numpy().reshape(Xt.shape[1:]), mean0)
    # S = 3 random rows: mean + A z, row by row
    A, mean = draw_matrix(rec, taxes, W, False)
    Z = np.random.default_rng(5).standard_normal((5, W))
    out3 = rec.sample(n_samples=3, z=Z[:3], jitter=CO.D, method="columns").reshape(3, M)
    ref = mean + Z[:3] @ A.T
    err = np.abs(out3 - ref).max()
    print("%s: S=3 draws - (mean + A z) = %.3e (bar %.3e)" % (name, err, 1e-11 * np.abs(out3).max()))
    assert err <= 1e-11 * np.abs(out3).max()
    # two calls with the same z give the same bits; a device tensor is the same call
    again = rec.sample(n_samples=3, z=Z[:3], jitter=CO.D, method="columns").reshape(3, M)
    assert np.array_equal(again, out3)
    assert np.array_equal(rec.sample(3, z=torch.from_numpy(Z[:3]).cuda(), jitter=CO.D, method="columns").reshape(3, M), out3)
    # grouping does not leak: S = 5 in one call against the same rows in calls of 2 and 3
    out5 = rec.sample(n_samples=5, z=Z, jitter=CO.D, method="columns").reshape(5, M)
    a = rec.sample(n_samples=2, z=Z[:2], jitter=CO.D, method="columns").reshape(2, M)
    b = rec.sample(n_samples=3, z=Z[2:], jitter=CO.D, method="columns").reshape(3, M)
    assert np.array_equal(out5, np.concatenate([a, b]))
    # seeded draws repeat; noiseless: nothing of z_n reaches the draw
    s1, s2 = rec.sample(3, seed=11, method="columns"), rec.sample(3, seed=11, method="columns")
    assert np.array_equal(s1, s2) and not np.array_equal(s1, rec.sample(3, seed=12, method="columns"))
    A0, _ = draw_matrix(rec, taxes, W, True)
    assert not A0[:, Us * U + N:].any() and A0[:, :Us * U + N].any()
    # predict() is what it was
    mean1, sd1 = rec.predict(Xt)
    assert np.array_equal(mean1, mean0) and np.array_equal(sd1, sd0)


@pytest.mark.parametrize("grid", ["half", None], ids=["own-union", "shared-union"])
def test_draw_groups_inside_one_call(grid, monkeypatch):
    """S = 10 draws in one group (GPIMHIP_PKRON_DRAW_GROUP unset: the budget holds thousands of draws of this cube) against
    groups of 4, 4 and 2 inside one call: a group that starts at s0 > 0, the mean computed by the first group alone and read
    by the later ones, a ragged last group.  The draws and the entry point's mean_out have the same bits."""
    from gpim_amd import _lib
    name = "6x5x4"
    rec, params = build(name, 0)
    taxes = axes_of(name, grid)
    Us, U, N, M = oracle(rec, params, taxes, False)[4]
    W = Us * U + N + M
    z = torch.from_numpy(np.random.default_rng(7).standard_normal((10, W))).to(rec._dev)

    def call(noiseless):
        mean = torch.zeros(M, dtype=torch.float64, device=rec._dev)
        out = torch.zeros((10, M), dtype=torch.float64, device=rec._dev)
        _lib.check(rec._solver.sample_columns(rec, taxes, z, noiseless, CO.D, mean, out))
        return out.cpu().numpy(), mean.cpu().numpy()

    for noiseless in (False, True):
        monkeypatch.delenv("GPIMHIP_PKRON_DRAW_GROUP", raising=False)
        one_out, one_mean = call(noiseless)
        monkeypatch.setenv("GPIMHIP_PKRON_DRAW_GROUP", "4")
        out, mean = call(noiseless)
        assert np.isfinite(one_out).all() and one_out.any() and not np.array_equal(one_out[0], one_out[9])
        assert np.array_equal(out, one_out) and np.array_equal(mean, one_mean)


def test_against_the_joint_draws_of_the_dense_model():
    """12 x 12 x 6: the dense engine's method='joint' on the same observations gives Sigma_post + (c_n + jitter) I; A A^T of
    method='columns' minus the oracle's extra term and c_n I must agree with it at 1e-7, the bar tests/test_gpu_columns.py
    holds this solver to against the dense engine."""
    import gpim_amd
    rec, params = build("12x12x6", 0)
    den, _ = build("12x12x6", 0, cls=gpim_amd.reconstructor)
    assert type(den._solver).__name__ == "Dense" and torch.equal(den._u, rec._u)
    taxes = axes_of("12x12x6", None)
    Xt = grid_of(taxes)
    j = 3e-4
    for noiseless in (False, True):
        _, _, cov, extra, (Us, U, N, M) = oracle(rec, params, taxes, noiseless, jitter=j)
        A, _ = draw_matrix(rec, taxes, Us * U + N + M, noiseless, jitter=j)
        out = den.sample(n_samples=M, Xtest=Xt, z=np.eye(M), noiseless=noiseless, jitter=j, method="joint")
        B = (out.reshape(M, M) - den.predict(Xt)[0].reshape(-1)).T
        cn = 0.0 if noiseless else params[2]
        err = np.abs((A @ A.T - extra - cn * np.eye(M)) - (B @ B.T - (cn + j) * np.eye(M))).max()
        print("12x12x6 noiseless=%d: max|Sigma_post (columns) - Sigma_post (joint)| = %.3e (bar 1e-7)" % (noiseless, err))
        assert err <= 1e-7


def test_refused_arguments_leave_the_model_alone():
    name = "6x5x4"
    rec, params = build(name, 0, iterations=1)             # (a model of its own: the accepted call at the end stores a grid)
    taxes = axes_of(name, "half")
    rec.predict(grid_of(taxes))
    Us, U, N, M = oracle(rec, params, taxes, False)[4]
    W = Us * U + N + M
    before = rec.sample(2, seed=3, method="columns")
    kept = (rec.Xtest, rec._Xtest_d, rec.fulldims, rec._solver.taxes)
    Xnan = grid_of(taxes)
    Xnan[0, 1, 2, 0] = np.nan
    Xbad = grid_of(taxes)
    Xbad[0, 3, 4, 1] += 0.25
    long_axis = grid_of([np.arange(2.0), np.arange(2.0), np.arange(4200.0) + 0.5])
    refusals = [
        (ValueError, "finite", dict(Xtest=Xnan)),
        (NotImplementedError, "product grid", dict(Xtest=Xbad)),
        (ValueError, "jitter", dict(jitter=0.0)),
        (ValueError, "jitter", dict(jitter=-1e-6)),
        (ValueError, "jitter", dict(jitter=float("inf"))),
        (ValueError, "n_samples", dict(n_samples=0)),
        (ValueError, "zeta.*z_e.*z_n", dict(z=np.zeros((2, M)))),
        (ValueError, "zeta.*%d.*%d.*%d" % (Us, N, M), dict(z=np.zeros((2, W - 1)))),
        (ValueError, "zeta", dict(z=np.zeros((3, W)))),
        (NotImplementedError, "axis 2.*420[0-9].*4096", dict(Xtest=long_axis)),
        (MemoryError, "GiB of device memory.*GiB are free", dict(n_samples=10 ** 8)),
        (ValueError, "method must be.*'kron' or 'columns'", dict(method="matheron")),
    ]
    for exc, match, kw in refusals:
        kw.setdefault("method", "columns")
        kw.setdefault("n_samples", 2)
        with pytest.raises(exc, match=match):
            rec.sample(seed=3, **kw)
        now = (rec.Xtest, rec._Xtest_d, rec.fulldims, rec._solver.taxes)
        assert all(a is b for a, b in zip(kept, now)), kw
        assert np.array_equal(rec.sample(2, seed=3, method="columns"), before), kw
    # the five other methods keep refusing this model, now naming the one it has
    for method in ("joint", "pathwise", "blocks", "border", "kron"):
        with pytest.raises(NotImplementedError, match="method='columns'"):
            rec.sample(1, method=method)
    # an accepted call with a new grid stores it, as predict() does
    own = grid_of(axes_of(name, None))
    out = rec.sample(2, seed=3, Xtest=own, method="columns")
    assert out.shape == (2, 6, 5, 4) and tuple(rec.fulldims) == (6, 5, 4) and rec._solver.taxes is not kept[3]


def test_refused_models():
    import gpim_amd
    from gpim_amd import _solvers
    Xg, X, R = data("12x12x6")
    full = np.nan_to_num(R)
    scattered = full.copy()
    scattered.ravel()[np.random.default_rng(0).choice(full.size, size=60, replace=False)] = np.nan
    Xsc = Xg.copy()
    Xsc[:, np.isnan(scattered)] = np.nan
    models = [
        (gpim_amd.skreconstructor(Xg, full, Xg, kernel="RBF", verbose=0), "method='kron'"),                 # Kronecker
        (gpim_amd.skreconstructor(Xsc, scattered, Xg, kernel="RBF", verbose=0), "method='border'|method='joint'"),
        (gpim_amd.reconstructor(X, R, Xg, kernel="RBF", verbose=0), "method='joint'"),                      # dense
    ]
    assert models[0][0].solver == "kronecker" and models[1][0].solver in ("border", "dense")
    for rec, match in models:
        with pytest.raises(NotImplementedError, match=match):
            rec.sample(2, seed=0, method="columns")
        with pytest.raises(NotImplementedError, match="solver='columns'"):
            rec._solver.sample_columns(rec)
    single = gpim_amd.skreconstructor(X, R, Xg, kernel="RBF", verbose=0, precision="single")
    if isinstance(single._solver, _solvers.Columns):
        with pytest.raises(NotImplementedError, match="single"):
            single.sample(2, seed=0, method="columns")


def test_cabi_misuse_leaves_the_handle_usable():
    """gpimhip_sample_pkron refuses every limit of its header before it allocates or launches anything; after each refusal
    a good call on the same handle gives the bits it gave before."""
    from gpim_amd import _lib
    from gpim_amd._lib import ptr
    rec, params = build("6x5x4", 0)
    sol, lib, h = rec._solver, rec._handle.lib, rec._handle.h
    taxes = axes_of("6x5x4", "half")
    rows, caxes, (P, iX, iT), (au, ic, it) = sol.sample_geometry(taxes)
    Us, U, N, M = oracle(rec, params, taxes, False)[4]
    W = Us * U + N + M
    i32 = lambda v: (ctypes.c_int32 * len(v))(*[int(k) for k in v])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(rec._dev)
    rows_d, caxes_d, P_d, au_d = dev(rows), dev(np.concatenate(caxes)), dev(P), dev(np.concatenate(au))
    z = torch.randn((2, W), dtype=torch.float64, device=rec._dev, generator=torch.Generator(rec._dev).manual_seed(1))
    mean, out = torch.empty(M, dtype=torch.float64, device=rec._dev), torch.empty((2, M), dtype=torch.float64, device=rec._dev)

    def call(handle=h, model=None, S=2, jitter=CO.D, iX_=iX, iT_=iT, nu=None, P_=None, z_=z):
        return lib.gpimhip_sample_pkron(
            handle, ctypes.byref(model or rec._mstruct), ptr(sol.Xs_d), sol.Xs_d.shape[0], 2, 1, sol.n_c, sol.perm,
            ptr(sol.axes_d), ptr(sol.Y_d), ptr(rec._u), ptr(rows_d), rows_d.shape[0], i32([len(c) for c in caxes]),
            ptr(caxes_d), ptr(P_d) if P_ is None else P_, P_d.shape[0], i32(iX_), i32(iT_),
            i32(nu or [len(a) for a in au]), ptr(au_d), i32(np.concatenate(ic)), i32(np.concatenate(it)),
            ptr(z_) if z_ is not None else None, S, 0, jitter, ptr(mean), ptr(out))

    assert call() == _lib.OK
    good = out.clone()
    bad_ix = iX.copy()
    bad_ix[3] = Us
    bad_it = iT.copy()
    bad_it[0] = -1
    H32 = _lib.Handle(precision="single")
    misuse = [
        (dict(z_=None), "null"), (dict(P_=ctypes.c_void_p(0)), "null"), (dict(S=0), "S >= 1"), (dict(jitter=0.0), "jitter"),
        (dict(jitter=float("nan")), "jitter"), (dict(jitter=float("inf")), "jitter"), (dict(iX_=bad_ix), "irow_train"),
        (dict(iT_=bad_it), "irow_test"), (dict(nu=[4200]), "axis 0.*4200.*4096"),
        (dict(handle=H32.h), "double-precision"),
    ]
    import re
    for kw, match in misuse:
        bytes0 = lib.gpimhip_workspace_bytes(h)
        assert call(**kw) == _lib.E_BADARG, kw
        assert re.search(match, lib.gpimhip_last_error().decode()), (kw, lib.gpimhip_last_error().decode())
        assert lib.gpimhip_workspace_bytes(h) == bytes0
        out.zero_()
        assert call() == _lib.OK and torch.equal(out, good), kw
    # reflection mode
    twoc = (ctypes.c_double * 4)(0, 0, 0, 0)
    assert lib.gpimhip_set_reflection(h, 1, twoc, None, N, 0) == _lib.OK
    assert call() == _lib.E_BADARG and "reflection" in lib.gpimhip_last_error().decode()
    assert lib.gpimhip_set_reflection(h, 0, twoc, None, 0, 0) == _lib.OK
    out.zero_()
    assert call() == _lib.OK and torch.equal(out, good)
