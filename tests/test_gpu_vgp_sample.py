"""
Joint posterior draws of the multi-output GP on the MI355X: gpimhip_sample_vgp,
gpimhip_sample_vgp_blocks and vreconstructor.sample against the host oracles of tests/vgp_sample_oracle.py -- the dense
N T posterior (mean, full covariance) and the block recipe on the same standard normals.  Device and oracle are both pure
functions of z; the oracle's eigenvectors come from the engine's own Jacobi iteration restated on the host, so the latent
blocks have the same order and signs on both sides.

Bar: atol 1e-10 on draws, covariances, means and variances, the bar of tests/test_gpu_sample.py for the single-output draws
(the host restatement reaches <= 2e-13, tests/test_vgp_sample_host.py).  Every test prints the figure it reaches.
"""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch
from numpy.testing import assert_allclose

pytestmark = pytest.mark.gpu

import pathwise_oracle as PO
import vgp_oracle as VO
import vgp_sample_oracle as VS

ATOL = 1e-10
JITTER = 1e-5
BOUNDS = ((0.5, 0.5), (2.5, 2.5))


def dev(t):
    return (torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t).cuda().contiguous()


def scattered(X, Y):
    N, d = X.shape
    dims = (N,) + (1,) * (d - 1)
    return np.ascontiguousarray(X.T).reshape((d,) + dims), Y.reshape(dims + (Y.shape[1],))


def model(X, Y, kernel, independent, bounds):
    """A vreconstructor on scattered rows: the holder of the handle and the two C structs."""
    import gpim_amd
    Xg, Yg = scattered(X, Y)
    return gpim_amd.vreconstructor(Xg, Yg, kernel=kernel, lengthscale=None if bounds is None else [bounds[0], bounds[1]],
                                   independent=independent, verbose=0, solver="dense")


def head(rec):
    return rec._handle.h, ctypes.byref(rec._mstruct), ctypes.byref(rec._vstruct)


def sample_rc(rec, Xd, Yd, ud, Xsd, Zd, noiseless, jitter, mean, var, out, S=None):
    from gpim_amd import _lib
    p = lambda t: None if t is None else _lib.ptr(t)
    return rec._handle.lib.gpimhip_sample_vgp(*head(rec), p(Xd), p(Yd), Xd.shape[0], p(ud), p(Xsd), Xsd.shape[0], p(Zd),
                                              Zd.shape[1] if S is None else S, int(noiseless), float(jitter), p(mean), p(var),
                                              p(out))


def sample_call(rec, Q, Z, noiseless, moments=True):
    """gpimhip_sample_vgp -> (draws (S, M, T), mean (M, T) or None, var or None) on the host"""
    from gpim_amd import _lib
    T, S, M = Z.shape
    out = torch.full((S, M, T), float("nan"), dtype=torch.float64, device="cuda")
    mean = torch.full((M, T), float("nan"), dtype=torch.float64, device="cuda") if moments else None
    var = torch.full((M, T), float("nan"), dtype=torch.float64, device="cuda") if moments else None
    _lib.check(sample_rc(rec, Q["Xd"], Q["Yd"], Q["ud"], Q["Xsd"], dev(Z), noiseless, JITTER, mean, var, out))
    return out.cpu().numpy(), (mean.cpu().numpy() if moments else None), (var.cpu().numpy() if moments else None)


def predict_call(rec, Xd, Yd, ud, Xsd):
    from gpim_amd import _lib
    M, T = Xsd.shape[0], Yd.shape[0]
    pm = torch.empty((M, T), dtype=torch.float64, device="cuda")
    pv = torch.empty_like(pm)
    _lib.check(rec._handle.lib.gpimhip_predict_vgp(*head(rec), _lib.ptr(Xd), _lib.ptr(Yd), Xd.shape[0], _lib.ptr(ud),
                                                   _lib.ptr(Xsd), M, _lib.ptr(pm), _lib.ptr(pv)))
    return pm.cpu().numpy(), pv.cpu().numpy()


def unit_probes(T, W):
    """Z (T, T W, W): draw t W + k has the unit vector e_k in block t and zeros elsewhere."""
    Z = np.zeros((T, T * W, W))
    for t in range(T):
        Z[t, t * W:(t + 1) * W] = np.eye(W)
    return Z


# (T, N, M, kernel, test points on the training points, noiseless, independent, bounds)
#   2 / 200 / 100: order 300 -> three 128-tiles with the K / K* boundary inside one; 16: GPIMHIP_VGP_MAX_TASKS
CASES = ((3, 150, 90, "RBF", False, 0, False, BOUNDS),
         (3, 150, 90, "Matern52", True, 1, True, BOUNDS),
         (2, 200, 100, "RBF", True, 1, False, None),
         (1, 130, 130, "Matern52", True, 0, False, BOUNDS),
         (16, 40, 24, "RBF", False, 0, False, BOUNDS))


def case_id(c):
    return "T%d-N%d-M%d-%s-%s-%s%s%s" % (c[0], c[1], c[2], c[3], "on" if c[4] else "off", "noiseless" if c[5] else "noisy",
                                         "-independent" if c[6] else "", "-softplus" if c[7] is None else "")


@functools.lru_cache(maxsize=None)
def problem(case):
    """Data, parameters and both oracles of one case, computed once."""
    T, N, M, kernel, on, noiseless, independent, bounds = case
    X, Y = VO.random_data(N, T, 2, seed=N + T)
    Xs = X[:M].copy() if on else np.random.default_rng(N).uniform(0.0, 8.0, size=(M, 2))
    u = VS.strong_u(T, 2, independent, seed=T + M)
    mean_d, Sig = VS.dense(u, X, Y, Xs, kernel, independent, bounds, noiseless, JITTER)
    R = VS.Recipe(u, X, Y, kernel, independent, bounds, eig="jacobi")
    J = R.joint(Xs, noiseless, JITTER)
    pm, pv = VO.Dense(X, Y, kernel, independent, bounds).predict(u, Xs)
    return dict(X=X, Y=Y, Xs=Xs, u=u, mean_d=mean_d, Sig=Sig, R=R, J=J, pm=pm, pv=pv)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_joint_route_against_the_dense_posterior(ensure_built, case):
    T, N, M, kernel, on, noiseless, independent, bounds = case
    Q = dict(problem(case))
    rec = model(Q["X"], Q["Y"], kernel, independent, bounds)
    Q.update(Xd=dev(Q["X"]), Yd=dev(np.ascontiguousarray(Q["Y"].T)), ud=dev(Q["u"]), Xsd=dev(Q["Xs"]))
    R, J = Q["R"], Q["J"]
    # ---- the factor from the T M unit vectors: D D^T = Sigma (with s_a jitter on its diagonal), mean and variance
    out, mean, var = sample_call(rec, Q, unit_probes(T, M), noiseless)
    A = (out - mean[None]).reshape(T * M, M * T).T
    pm, pv = predict_call(rec, Q["Xd"], Q["Yd"], Q["ud"], Q["Xsd"])
    figs = dict(cov=np.abs(A @ A.T - Q["Sig"]).max(), mean_predict=np.abs(mean - pm).max(), var_predict=np.abs(var - pv).max(),
                mean_dense=np.abs(mean - Q["pm"]).max(), var_dense=np.abs(var - Q["pv"]).max(),
                mean_posterior=np.abs(mean - Q["mean_d"]).max(), factor=np.abs(A - R.joint_factor(J)).max())
    print("%s: lambda max %.1f; " % (case_id(case), R.lam.max()) + ", ".join("%s %.2e" % kv for kv in figs.items()))
    assert np.isfinite(out).all()
    for k, v in figs.items():
        assert v <= ATOL, (k, v)
    # ---- seeded draws: mean + D z, and the recipe oracle
    for S in (1, 3, 16, 17):
        Z = np.random.default_rng(10 + S).standard_normal((T, S, M))
        o, m2, v2 = sample_call(rec, Q, Z, noiseless)
        want = mean[None] + (Z.transpose(1, 0, 2).reshape(S, T * M) @ A.T).reshape(S, M, T)
        ref = R.joint_draws(J, Z)
        print("%s S=%d: draws - (mean + D z) %.2e, draws - oracle %.2e"
              % (case_id(case), S, np.abs(o - want).max(), np.abs(o - ref).max()))
        assert_allclose(o, want, rtol=0, atol=ATOL)
        assert_allclose(o, ref, rtol=0, atol=ATOL)
        assert np.array_equal(m2, mean) and np.array_equal(v2, var)
        # null mean / var outputs: the same draws bit for bit; a second identical call as well
        assert np.array_equal(sample_call(rec, Q, Z, noiseless, moments=False)[0], o)
        assert np.array_equal(sample_call(rec, Q, Z, noiseless)[0], o)


# ------------------------------------------------------------------------------------------ blocks route
GRIDS = (((8, 7), 3, "RBF"), ((6, 6), 2, "Matern52"), ((5, 4, 4), 2, "RBF"))


def grid_problem(shape, T, seed=0):
    Xg, G = PO.full_grid(shape)
    rng = np.random.default_rng(seed + len(G))
    base = np.stack([np.sin(G @ rng.normal(size=len(shape)) * 0.5 + rng.uniform(0, 6)) for _ in range(3)], 1)
    Y = base @ rng.normal(size=(3, T)) + 0.1 * rng.normal(size=(len(G), T)) + rng.normal(size=T)
    return Xg, G, Y


def blocks_rc(rec, blocks, Gd, Yd, ud, Zd, noiseless, jitter, mean, out, mask=None, S=None):
    from gpim_amd import _lib
    p = lambda t: None if t is None else _lib.ptr(t)
    shape = (ctypes.c_int32 * blocks.d)(*blocks.shape)
    mask = sum(1 << k for k in blocks.dims) if mask is None else mask
    twoc = (ctypes.c_double * 4)(*(list(blocks.S["twoc"])))
    return rec._handle.lib.gpimhip_sample_vgp_blocks(*head(rec), p(Gd), shape, mask, twoc, p(Yd), p(ud), p(Zd),
                                                     Zd.shape[1] if S is None else S, int(noiseless), float(jitter), p(mean),
                                                     p(out))


def blocks_call(rec, blocks, Gd, Yd, ud, Z, noiseless, want_mean=True):
    from gpim_amd import _lib
    T, S, M = Z.shape[0], Z.shape[1], blocks.M
    out = torch.full((S, M, T), float("nan"), dtype=torch.float64, device="cuda")
    mean = torch.full((M, T), float("nan"), dtype=torch.float64, device="cuda") if want_mean else None
    _lib.check(blocks_rc(rec, blocks, Gd, Yd, ud, dev(Z), noiseless, JITTER, mean, out))
    return out.cpu().numpy(), (mean.cpu().numpy() if want_mean else None)


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(str(n) for n in g[0]))
def test_blocks_route_against_the_dense_posterior(ensure_built, grid):
    shape, T, kernel = grid
    d = len(shape)
    Xg, G, Y = grid_problem(shape, T)
    M = len(G)
    blocks = PO.Blocks(Xg)
    bounds = ([0.5] * d, [2.5] * d)
    u = VS.strong_u(T, d, False, seed=M)
    R = VS.Recipe(u, G, Y, kernel, False, bounds, eig="jacobi")
    rec = model(G, Y, kernel, False, bounds)
    Gd, Yd, ud = dev(G), dev(np.ascontiguousarray(Y.T)), dev(u)
    pm, _ = predict_call(rec, Gd, Yd, ud, Gd)
    for noiseless in (1, 0):
        W = 2 * M + (0 if noiseless else M)
        Z = np.random.default_rng(20 + noiseless).standard_normal((T, 3, W))
        out, mean = blocks_call(rec, blocks, Gd, Yd, ud, Z, noiseless)
        ref = R.blocks_draws(blocks, Z, bool(noiseless), JITTER)
        print("%s T=%d noiseless=%d: draws - oracle %.2e, mean - predict %.2e, mean - oracle %.2e"
              % ("x".join(map(str, shape)), T, noiseless, np.abs(out - ref["out"]).max(), np.abs(mean - pm).max(),
                 np.abs(mean - ref["mean"]).max()))
        assert np.isfinite(out).all()
        assert_allclose(out, ref["out"], rtol=0, atol=ATOL)
        assert_allclose(mean, pm, rtol=0, atol=ATOL)
        assert_allclose(mean, ref["mean"], rtol=0, atol=ATOL)
        assert np.array_equal(blocks_call(rec, blocks, Gd, Yd, ud, Z, noiseless, want_mean=False)[0], out)
    # the covariance from the unit vectors over the 2 M columns of every block
    mean_d, Sig = VS.dense_blocks(u, G, Y, kernel, False, bounds, True, JITTER)
    out, mean = blocks_call(rec, blocks, Gd, Yd, ud, unit_probes(T, 2 * M), 1)
    A = (out - mean[None]).reshape(T * 2 * M, M * T).T
    err = np.abs(A @ A.T - Sig).max()
    print("%s T=%d: |A A^T - Sigma| %.2e, mean - dense %.2e" % ("x".join(map(str, shape)), T, err, np.abs(mean - mean_d).max()))
    assert err <= ATOL
    assert_allclose(mean, mean_d, rtol=0, atol=ATOL)


# ------------------------------------------------------------------------------------------ refusals, workspace
def test_bad_arguments_leave_the_handle_usable(ensure_built):
    from gpim_amd import _lib
    shape, T = (8, 7), 3
    Xg, G, Y = grid_problem(shape, T)
    M = len(G)
    blocks = PO.Blocks(Xg)
    u = VS.strong_u(T, 2, False, seed=M)
    rec = model(G, Y, "RBF", False, BOUNDS)
    h = rec._handle
    shape_c = (ctypes.c_int32 * 2)(*shape)
    twoc = (ctypes.c_double * 4)(*(list(blocks.S["twoc"])))
    out = torch.empty((1, M, T), dtype=torch.float64, device="cuda")
    good = dict(G=dev(G), Y=dev(np.ascontiguousarray(Y.T)), u=dev(u), Zj=dev(np.zeros((T, 1, M))), Zb=dev(np.zeros((T, 1, 2 * M))),
                out=out)

    def joint(S=1, jitter=JITTER, r=rec, vg=None, **kw):
        a = {k: (None if v is None else _lib.ptr(v)) for k, v in dict(good, **kw).items()}
        return r._handle.lib.gpimhip_sample_vgp(r._handle.h, ctypes.byref(r._mstruct), ctypes.byref(vg or r._vstruct), a["G"], a["Y"],
                                                M, a["u"], a["G"] if "Xs" not in kw else a["Xs"], M, a["Zj"], S, 1, jitter, None,
                                                None, a["out"])

    def blk(S=1, jitter=JITTER, mask=3, r=rec, vg=None, shp=shape_c, tc=twoc, **kw):
        a = {k: (None if v is None else _lib.ptr(v)) for k, v in dict(good, **kw).items()}
        return r._handle.lib.gpimhip_sample_vgp_blocks(r._handle.h, ctypes.byref(r._mstruct), ctypes.byref(vg or r._vstruct),
                                                       a["G"], shp, mask, tc, a["Y"], a["u"], a["Zb"], S, 1, jitter, None, a["out"])

    assert joint() == _lib.OK
    first = out.cpu().numpy().copy()
    assert blk() == _lib.OK
    # null pointers, no draws, a jitter that is not positive
    for kw in (dict(G=None), dict(Y=None), dict(u=None), dict(Xs=None), dict(Zj=None), dict(out=None), dict(S=0), dict(S=-1),
               dict(jitter=0.0), dict(jitter=-1e-9), dict(jitter=float("nan"))):
        assert joint(**kw) == _lib.E_BADARG, kw
    for kw in (dict(G=None), dict(Y=None), dict(u=None), dict(Zb=None), dict(out=None), dict(shp=None), dict(tc=None), dict(S=0),
               dict(jitter=0.0), dict(jitter=-1e-9), dict(jitter=float("nan")), dict(jitter=1.0 + 1e-9), dict(mask=0),
               dict(mask=4)):
        assert blk(**kw) == _lib.E_BADARG, kw
    assert blk(jitter=2.0) == _lib.E_BADARG and b"jitter <= 1" in h.lib.gpimhip_last_error()
    assert blk(mask=0) == _lib.E_BADARG and b"reflected axis" in h.lib.gpimhip_last_error()
    assert blk(jitter=1.0) == _lib.OK
    # more than GPIMHIP_VGP_MAX_TASKS tasks
    vg = _lib.VgpStruct()
    vg.tasks, vg.rank, vg.independent, vg.ls_softplus = 17, 1, 0, 0
    big = dict(Y=dev(np.zeros((17, M))), Zj=dev(np.zeros((17, 1, M))), Zb=dev(np.zeros((17, 1, 2 * M))),
               u=dev(np.zeros(VO.layout(17, 2, False)[1])), out=torch.empty((1, M, 17), dtype=torch.float64, device="cuda"))
    assert joint(vg=vg, **big) == _lib.E_BADARG and blk(vg=vg, **big) == _lib.E_BADARG
    # a handle in reflection mode
    mode = types.SimpleNamespace(mask=3, twoc=(ctypes.c_double * 4)(7.0, 6.0, 0.0, 0.0), wts=None, n_total=M)
    with _lib.reflection(h, mode):
        assert joint() == _lib.E_BADARG
        assert b"gpimhip_sample_vgp: not available in reflection mode" in h.lib.gpimhip_last_error()
        assert blk() == _lib.E_BADARG
        assert b"gpimhip_sample_vgp_blocks: not available in reflection mode" in h.lib.gpimhip_last_error()
    # single precision
    H32 = _lib.Handle(precision="single")
    try:
        r32 = types.SimpleNamespace(_handle=H32, _mstruct=rec._mstruct, _vstruct=rec._vstruct)
        assert joint(r=r32) == _lib.E_BADARG and blk(r=r32) == _lib.E_BADARG
    finally:
        H32.close()
    # the handle still draws, the same bits
    assert blk() == _lib.OK and joint() == _lib.OK
    assert np.array_equal(out.cpu().numpy(), first)


def test_nothing_else_moves(ensure_built):
    """A draw uses matrices of its own: the workspace of fit / predict keeps its contents and its size."""
    from gpim_amd import _lib
    T, N, M = 3, 300, 129
    X, Y = VO.random_data(N, T, 2, seed=5)
    Xs = np.random.default_rng(1).uniform(0.0, 8.0, size=(M, 2))
    u = VS.strong_u(T, 2, False, seed=9)
    Xd, Yd, Xsd = dev(X), dev(np.ascontiguousarray(Y.T)), dev(Xs)
    Z = np.random.default_rng(2).standard_normal((T, 3, M))

    def fit(rec):
        ud = dev(u.copy())
        hist = torch.empty((5, 2), dtype=torch.float64, device="cuda")
        loss = torch.empty(5, dtype=torch.float64, device="cuda")
        _lib.check(rec._handle.lib.gpimhip_fit_vgp(*head(rec), _lib.ptr(Xd), _lib.ptr(Yd), N, _lib.ptr(ud), 0.05, 5, _lib.ptr(hist),
                                                   _lib.ptr(loss)))
        return hist.cpu(), loss.cpu(), ud.cpu()

    rec, rec2 = model(X, Y, "Matern52", False, BOUNDS), model(X, Y, "Matern52", False, BOUNDS)
    Q = dict(Xd=Xd, Yd=Yd, ud=dev(u), Xsd=Xsd)
    nbytes = lambda: rec._handle.lib.gpimhip_workspace_bytes(rec._handle.h)
    before = predict_call(rec, Xd, Yd, Q["ud"], Xsd)
    bytes0 = nbytes()
    s1 = sample_call(rec, Q, Z, 0)
    bytes1 = nbytes()
    s2 = sample_call(rec, Q, Z, 0)
    assert bytes1 > bytes0 and nbytes() == bytes1               # counted, and no growth at the same sizes
    assert all(np.array_equal(a, b) for a, b in zip(s1, s2))
    after = predict_call(rec, Xd, Yd, Q["ud"], Xsd)
    assert nbytes() == bytes1                                   # the training workspace was neither freed nor resized
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    got, fresh = fit(rec), fit(rec2)
    assert all(torch.equal(a, b) for a, b in zip(got, fresh))


# ------------------------------------------------------------------------------------------ Python surface
def stack12(seed=0):
    rng = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(12), np.arange(12), indexing="ij")
    base = np.stack([np.sin(ii / 3.0) * np.cos(jj / 4.0), np.cos(ii / 5.0 + jj / 3.0)], -1)
    return base @ rng.normal(size=(2, 3)) + 0.05 * rng.standard_normal((12, 12, 3))


LS = [[1., 1.], [8., 8.]]


def surface_model(solver):
    import gpim_amd
    Y = stack12()
    Xf = gpim_amd.utils.get_full_grid(Y[..., 0])
    X = Xf.astype(np.float64)
    if solver == "border":
        Y = Y.copy()
        for hole in ((3, 4), (9, 2), (6, 6)):
            Y[hole] = np.nan
            X[(slice(None),) + hole] = np.nan
    rec = gpim_amd.vreconstructor(X, Y, kernel="Matern52", lengthscale=LS, learning_rate=0.1, iterations=5, verbose=0,
                                  solver=solver)
    assert rec.solver == solver
    rec.train()
    return rec, Xf, Y


def surface_oracle(rec):
    return VS.Recipe(rec._u.cpu().numpy(), rec.X.numpy(), rec.y.numpy(), "Matern52", False, (np.array(LS[0]), np.array(LS[1])),
                     eig="jacobi")


@pytest.mark.parametrize("solver", ("dense", "reflection", "border"))
def test_vreconstructor_sample(ensure_built, solver):
    rec, Xf, Y = surface_model(solver)
    N = rec.X.shape[0]
    assert N == (141 if solver == "border" else 144)
    R = surface_oracle(rec)
    for noiseless in (False, True):
        z = torch.randn((3, 3, 144), dtype=torch.float64, device=rec._dev, generator=torch.Generator(rec._dev).manual_seed(1))
        got = rec.sample(n_samples=3, Xtest=Xf, z=z, noiseless=noiseless)
        assert got.shape == (3, 12, 12, 3) and got.dtype == np.float64 and np.isfinite(got).all()
        ref = R.joint_draws(R.joint(Xf.reshape(2, -1).T, noiseless, 1e-5), z.cpu().numpy()).reshape(3, 12, 12, 3)
        print("%s noiseless=%d: sample - oracle %.2e" % (solver, noiseless, np.abs(got - ref).max()))
        assert_allclose(got, ref, rtol=0, atol=ATOL)
        assert np.array_equal(got, rec.sample(n_samples=3, seed=1, noiseless=noiseless))        # the stored grid, the same z
        assert np.array_equal(got, rec.sample(n_samples=3, z=z.cpu().numpy(), noiseless=noiseless))
    a = rec.sample(n_samples=3, seed=1)
    assert np.array_equal(a, rec.sample(n_samples=3, seed=1)) and not np.array_equal(a, rec.sample(n_samples=3, seed=2))
    assert not np.array_equal(a, rec.sample(n_samples=3, seed=1, noiseless=True))
    assert rec.sample().shape == (1, 12, 12, 3)
    # the training points as the test grid
    rec.Xtest = None
    with pytest.warns(UserWarning):
        rows = rec.sample(n_samples=3, seed=1)
    assert rows.shape == (3, N, 3)
    rec.predict(Xf, verbose=0)
    # refusals leave the stored grid as it was
    grid = (rec.Xtest, rec.fulldims)
    with pytest.raises(NotImplementedError, match="'joint'.*'blocks'"):
        rec.sample(method="pathwise")
    with pytest.raises(NotImplementedError, match="'joint'.*'blocks'"):
        rec.sample(method="border")
    with pytest.raises(ValueError, match="method must be"):
        rec.sample(method="matheron")
    Xnan = Xf.astype(np.float64)
    Xnan[:, 3, 4] = np.nan
    with pytest.raises(ValueError, match="finite"):
        rec.sample(Xtest=Xnan)
    for bad in (np.zeros((3, 144)), np.zeros((3, 3, 143)), np.zeros((3, 2, 144))):
        with pytest.raises(ValueError, match=r"\(T, n_samples, W\)"):
            rec.sample(n_samples=3, z=bad)
    with pytest.raises(ValueError, match="jitter"):
        rec.sample(jitter=0.0)
    assert rec.Xtest is grid[0] and rec.fulldims == grid[1]
    # method='blocks'
    if solver == "border":
        with pytest.raises(NotImplementedError, match=r"grid point \(3, 4\) has none"):
            rec.sample(method="blocks")
    else:
        zb = torch.randn((3, 2, 3 * 144), dtype=torch.float64, device=rec._dev, generator=torch.Generator(rec._dev).manual_seed(3))
        got = rec.sample(n_samples=2, z=zb, method="blocks")
        assert got.shape == (2, 12, 12, 3)
        blocks = PO.Blocks(Xf.astype(np.float64))
        ref = R.blocks_draws(blocks, zb.cpu().numpy(), False, 1e-5)["out"].reshape(2, 12, 12, 3)
        mean, _ = rec.predict(verbose=0)
        at0 = rec.sample(n_samples=1, z=np.zeros((3, 1, 3 * 144)), method="blocks")[0]
        print("%s blocks: sample - oracle %.2e, sample(z = 0) - predict %.2e"
              % (solver, np.abs(got - ref).max(), np.abs(at0 - mean).max()))
        assert_allclose(got, ref, rtol=0, atol=ATOL)
        assert_allclose(at0, mean, rtol=0, atol=ATOL)
        assert np.array_equal(rec.sample(n_samples=2, seed=3, method="blocks"), got)
        with pytest.raises(ValueError, match="jitter"):
            rec.sample(method="blocks", jitter=1.5)
        with pytest.raises(ValueError, match=r"\(T, n_samples, W\)"):
            rec.sample(n_samples=2, z=np.zeros((3, 2, 144)), method="blocks")
        fine = np.array(np.meshgrid(np.arange(0.0, 11.5, 0.5), np.arange(0.0, 11.5, 0.5), indexing="ij"))
        with pytest.raises(NotImplementedError, match=r"grid point \(0, 1\) has none"):
            rec.sample(Xtest=fine, method="blocks")
        with pytest.raises(NotImplementedError, match="not on it"):
            rec.sample(Xtest=Xf + 0.5, method="blocks")
    assert rec.Xtest is grid[0] and rec.fulldims == grid[1]
    mean, sd = rec.predict(verbose=0)
    assert mean.shape == (12, 12, 3) and np.isfinite(mean).all() and np.isfinite(sd).all()


def test_training_goes_on_after_a_draw(ensure_built):
    """solver='reflection': 3 iterations, a draw, 3 more -- the same history bits as 3 + 3 without the draw, and the handle's
    workspace is the size it was (the draw has its own)."""
    import gpim_amd
    Y = stack12(1)
    Xf = gpim_amd.utils.get_full_grid(Y[..., 0])
    runs = []
    for draw in (True, False):
        rec = gpim_amd.vreconstructor(Xf, Y, kernel="Matern52", lengthscale=LS, learning_rate=0.1, iterations=3, verbose=0,
                                      solver="reflection")
        rec.train()
        if draw:
            rec.sample(n_samples=2, seed=0, Xtest=Xf)
            rec.sample(n_samples=2, seed=0, Xtest=Xf, method="blocks")
        rec.train()
        runs.append((np.array(rec.hyperparams["lengthscale"]), np.array(rec.loss_all), rec._u.cpu().numpy()))
    assert runs[0][0].shape == (6, 2)
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
