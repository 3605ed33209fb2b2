"""
Believer batches of CB / EI / POI on the MI355X (gpimhip_acquire_batch, reconstructor.acq_batch,
boptimizer(acq_batch='believer')) against the float64 scheme of tests/believer_oracle.py (`scheme`: the conditioned columns
from W = L^-1 K(X, G) in numpy), which tests/test_believer_host.py holds to literal refits at 1e-12.

Cases: the (kind, N, grid, q) of tests/ivr_greedy_oracle.py, each with CB(0, 1), CB(1, 2), EI and POI at xi = 0.01
(noise_u = -3, jitter 1e-5).  What the shapes reach: less than one 128-column strip (6 x 5); two strips, the second holding
2 columns (13 x 10); d = 3; five strips with a partial last one (25 x 25); N = 530: np = 640, a ragged last block and five
row chunks; N = 4 with 32 rounds: 31 correction terms.

Bars, per case:
  picks       equal to the oracle's, exactly: the host test shows every round's best value leading the second best by >= 1e-7
              relative, a thousand times the bar on the maps, so an engine inside that bar cannot flip one
  maps, vals  max |gpu - ref| <= 1e-10 max |round-0 reference map|, at the entries that are not NaN (the bar of
              tests/test_gpu_ivr_greedy.py)
  NaN         in row r exactly at the picks of the rounds before r
  sd_after^2  against predict's variance of the dense oracle refitted with the whole batch: <= 1e-10 relative
Every test prints the distances it measured before it asserts.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ivr_oracle as IO
import believer_oracle as BO
from test_gpu_ivr import ivr_abi, image16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-10
NAMES = ("idx", "val", "count", "maps", "mean", "sd", "sd_after")
GRID = [(c, s) for c in BO.CASES for s in BO.SETTINGS]
EI = BO.SETTINGS[2]


@pytest.fixture(scope="module")
def eng(ensure_built):
    from gpim_amd import _lib
    H = _lib.Handle()
    yield _lib, H
    H.close()


def abi_args(_lib, setting):
    """(kind id, p0, p1) of the entry for a setting (acquisition, p0, p1, xi)"""
    acqf, p0, p1, xi = setting
    return (_lib.ACQ_IDS[acqf],) + ((p0, p1) if acqf == "cb" else (0.0, xi))


def believer_abi(_lib, H, spec, u, X, y, G, q, setting, mask=None, want=True):
    """dict of numpy arrays (NAMES) of gpimhip_acquire_batch on the handle H, the observed rows being the training rows;
    maps and sd_after None without `want`"""
    M = G.shape[0]
    m = spec.struct()
    Xd, yd, ud, Gd = X.cuda().contiguous(), y.cuda().contiguous(), u.cuda(), G.cuda().contiguous()
    md = None if mask is None else torch.as_tensor(mask, dtype=torch.float64).cuda().contiguous()
    # three sentinels behind every output
    f = lambda n: torch.full((n + 3,), -7.0, dtype=torch.float64, device="cuda")
    val, maps, mean, sd, after = f(q), f(q * M), f(M), f(M), f(M)
    idx = torch.full((q + 3,), -7, dtype=torch.int64, device="cuda")
    count = torch.full((1 + 3,), -7, dtype=torch.int64, device="cuda")
    opt = lambda t: _lib.ptr(t) if want else None
    kind, p0, p1 = abi_args(_lib, setting)
    _lib.check(H.lib.gpimhip_acquire_batch(H.h, ctypes.byref(m), _lib.ptr(Xd), _lib.ptr(yd), X.shape[0], _lib.ptr(ud),
                                           _lib.ptr(Gd), M, _lib.ptr(Xd), X.shape[0], kind, p0, p1, _lib.ptr(md), q,
                                           _lib.ptr(mean), _lib.ptr(sd), opt(maps), opt(after), _lib.ptr(idx), _lib.ptr(val),
                                           _lib.ptr(count)))
    out = {}
    for name, t, n in (("idx", idx, q), ("val", val, q), ("count", count, 1), ("maps", maps, q * M), ("mean", mean, M),
                       ("sd", sd, M), ("sd_after", after, M)):
        h = t.cpu().numpy()
        assert np.all(h[n:] == -7), name
        out[name] = h[:n] if want or name not in ("maps", "sd_after") else None
    if want:
        out["maps"] = out["maps"].reshape(q, M)
    return out


def same_bits(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k], equal_nan=True) for k in NAMES)


def check_against(tag, got, ref, q, M, after_ref=None):
    """the bars of the module docstring, for the rounds the oracle made"""
    n = len(ref.picks)
    top = np.nanmax(np.abs(ref.maps[0])) if n else 1.0
    on = ~np.isnan(ref.maps)
    gap = np.abs(got["maps"][:n] - ref.maps)[on].max() if n else 0.0
    vgap = np.abs(got["val"][:n] - ref.vals).max() if n else 0.0
    print("%s: picks %s (oracle %s), max |map 0| %.4g, maps: max |gpu - ref| %.2e = %.2e of it, vals: %.2e = %.2e of it; "
          "smallest oracle gap %.2e" % (tag, got["idx"].tolist(), ref.picks.tolist(), top, gap, gap / top, vgap, vgap / top,
                                        ref.gaps.min() if n else np.inf))
    assert got["count"][0] == n
    assert np.array_equal(got["idx"][:n], ref.picks) and np.all(got["idx"][n:] == -1) and np.isnan(got["val"][n:]).all()
    assert np.array_equal(np.isnan(got["maps"][:n]), ~on) and np.isnan(got["maps"][n:]).all()
    assert gap <= BAR * top and vgap <= BAR * top
    assert np.isfinite(got["mean"]).all() and np.isfinite(got["sd"]).all() and np.isfinite(got["sd_after"]).all()
    if after_ref is not None:
        rel = np.abs(got["sd_after"] ** 2 / after_ref - 1.0).max()
        print("    sd_after^2 against the refit's predict: max rel %.2e" % rel)
        assert rel <= BAR


@pytest.mark.parametrize("case,setting", GRID, ids=[BO.ident(c, s) for c, s in GRID])
def test_against_oracle(eng, case, setting):
    _lib, H = eng
    kind, N, shape, q = case
    kp, spec, u, X, y, G = IO.case(kind, N, shape)
    M = G.shape[0]
    assert len(X) == N
    ref = BO.reference(*case, *setting)
    assert len(ref.picks) == q
    got = believer_abi(_lib, H, spec, u, X, y, G, q, setting)
    check_against(BO.ident(case, setting), got, ref, q, M, after_ref=BO.refit_variance(kp, X, G, ref.picks))
    # every pick lowers every variance
    assert (got["sd_after"] <= got["sd"]).all()


def acquire_abi(_lib, H, spec, u, X, y, G, setting):
    """(acq, mean, sd) of gpimhip_acquire_exact with the training rows as the observed rows"""
    M, m = G.shape[0], spec.struct()
    Xd, yd, ud, Gd = X.cuda().contiguous(), y.cuda().contiguous(), u.cuda(), G.cuda().contiguous()
    acq, mean, sd = (torch.empty(M, dtype=torch.float64, device="cuda") for _ in range(3))
    kind, p0, p1 = abi_args(_lib, setting)
    _lib.check(H.lib.gpimhip_acquire_exact(H.h, ctypes.byref(m), _lib.ptr(Xd), _lib.ptr(yd), X.shape[0], _lib.ptr(ud),
                                           _lib.ptr(Gd), M, _lib.ptr(Xd), X.shape[0], kind, p0, p1, None, _lib.ptr(mean),
                                           _lib.ptr(sd), _lib.ptr(acq)))
    return acq.cpu().numpy(), mean.cpu().numpy(), sd.cpu().numpy()


def test_round_zero_is_todays_acquisition(eng):
    """N = 530 (the K* slab path of predict): mean_out has the bits of gpimhip_predict_exact -- the same launch on the same
    slab; N = 530 and N = 130 (gpimhip_acquire_exact's fused launch): row 0 of the maps and sd_out are within the bar of
    gpimhip_acquire_exact; at q = 1 the pick is gpimhip_topk's first of that map."""
    _lib, H = eng
    for N, shape in ((530, (20, 15)), (130, (13, 10))):
        kp, spec, u, X, y, G = IO.case("Matern52", N, shape)
        M, m = G.shape[0], spec.struct()
        for setting in BO.SETTINGS:
            got = believer_abi(_lib, H, spec, u, X, y, G, 1, setting)
            acq, mean, sd = acquire_abi(_lib, H, spec, u, X, y, G, setting)
            top = np.abs(acq).max()
            print("N=%d %s: row 0 vs acquire_exact %.2e of max |map|, sd^2 rel %.2e, mean abs %.2e"
                  % (N, setting, np.abs(got["maps"][0] - acq).max() / top, np.abs(got["sd"] ** 2 / sd ** 2 - 1).max(),
                     np.abs(got["mean"] - mean).max()))
            assert np.abs(got["maps"][0] - acq).max() <= BAR * top
            assert np.abs(got["sd"] ** 2 / sd ** 2 - 1).max() <= BAR and np.abs(got["mean"] - mean).max() <= BAR
            ad = torch.from_numpy(got["maps"][0].copy()).cuda()
            vals, idx, cnt = (torch.zeros(1, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"),
                              torch.zeros(1, dtype=torch.int64, device="cuda"))
            _lib.check(H.lib.gpimhip_topk(H.h, _lib.ptr(ad), M, 1, 0, _lib.ptr(vals), _lib.ptr(idx), _lib.ptr(cnt)))
            assert got["count"][0] == 1 and got["idx"][0] == idx.item() and got["val"][0] == vals.item()
        if N == 530:
            Xd, yd, ud, Gd = X.cuda().contiguous(), y.cuda().contiguous(), u.cuda(), G.cuda().contiguous()
            pm, pv = (torch.empty(M, dtype=torch.float64, device="cuda") for _ in range(2))
            _lib.check(H.lib.gpimhip_predict_exact(H.h, ctypes.byref(m), _lib.ptr(Xd), _lib.ptr(yd), N, _lib.ptr(ud), _lib.ptr(Gd),
                                                   M, _lib.ptr(pm), _lib.ptr(pv)))
            assert np.array_equal(got["mean"], pm.cpu().numpy())


def test_two_calls_same_bits_and_ivr_untouched(eng):
    """Two calls give identical bits in every output, with and without the optional outputs; gpimhip_ivr_exact after a
    believer call (which shares W with it) returns the bits of a fresh handle."""
    _lib, H = eng
    kp, spec, u, X, y, G = IO.case("Matern52", 300, (25, 25))
    for setting in BO.SETTINGS:
        a = believer_abi(_lib, H, spec, u, X, y, G, 8, setting)
        b = believer_abi(_lib, H, spec, u, X, y, G, 8, setting)
        assert same_bits(a, b), setting
        c = believer_abi(_lib, H, spec, u, X, y, G, 8, setting, want=False)
        assert np.array_equal(c["idx"], a["idx"]) and np.array_equal(c["val"], a["val"]) and c["count"][0] == 8
        assert np.array_equal(c["mean"], a["mean"]) and np.array_equal(c["sd"], a["sd"]) and c["maps"] is None
    fresh = _lib.Handle()
    try:
        e0 = ivr_abi(_lib, fresh, spec, u, X, y, G)
    finally:
        fresh.close()
    e1 = ivr_abi(_lib, H, spec, u, X, y, G)
    assert all(np.array_equal(p, q) for p, q in zip(e0, e1))


def child_eval(out):
    """(run in a fresh process) the N = 530 case with EI on a new handle, saved to `out`"""
    from gpim_amd import _build, _lib
    _build.build()
    H = _lib.Handle()
    kp, spec, u, X, y, G = IO.case("Matern52", 530, (20, 15))
    got = believer_abi(_lib, H, spec, u, X, y, G, 6, EI)
    np.savez(out, **got)
    H.close()


def test_chunked_slab_same_bits(eng, tmp_path):
    """GPIMHIP_PREDICT_CHUNK=128 in a fresh process: W (and the incumbent's posterior) assembled from slabs of one tile
    each, the second and the ragged last one included -- the bits of the unchunked call."""
    _lib, H = eng
    out = str(tmp_path / "chunked.npz")
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_believer as t; t.child_eval(%r)"
            % (ROOT, os.path.join(ROOT, "tests"), out))
    env = dict(os.environ, GPIMHIP_PREDICT_CHUNK="128")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    kp, spec, u, X, y, G = IO.case("Matern52", 530, (20, 15))
    whole = believer_abi(_lib, H, spec, u, X, y, G, 6, EI)
    with np.load(out) as z:
        chunked = {k: z[k] for k in NAMES}
    for k in NAMES:
        print(k, "chunked vs whole: max |diff|", np.nanmax(np.abs(chunked[k].astype(np.float64) - whole[k])))
    assert same_bits(chunked, whole)
    assert np.array_equal(whole["idx"], BO.reference("Matern52", 530, (20, 15), 6, *EI).picks)


def test_ragged_block_and_stale_padding(eng):
    """A handle that fitted N = 600 (every row of the workspace written) and ran a believer batch of that order returns at
    N = 530 (np = 640, 18 valid rows in the last block) the bits of a fresh handle."""
    _lib, H = eng
    from gpim_amd.kernels import KernelSpec
    kp, spec, u, X, y, G = IO.case("Matern52", 530, (20, 15))
    fresh, used = _lib.Handle(), _lib.Handle()
    try:
        X6, y6 = IO.scattered(600, 2, seed=600, grid=64)
        s6 = KernelSpec("RBF", 2, [[1., 1.], [20., 20.]], jitter=1e-5)
        u6 = s6.draw_initial_u(generator=torch.Generator().manual_seed(6)).cuda()
        m6 = s6.struct()
        X6d, y6d = X6.cuda().contiguous(), y6.cuda().contiguous()
        _lib.check(used.lib.gpimhip_fit_exact(used.h, ctypes.byref(m6), _lib.ptr(X6d), _lib.ptr(y6d), len(X6), _lib.ptr(u6), 0.1,
                                              3, None, None))
        believer_abi(_lib, used, s6, u6.cpu(), X6, y6, G, 6, EI)
        for setting in BO.SETTINGS:
            b = believer_abi(_lib, fresh, spec, u, X, y, G, 6, setting)
            c = believer_abi(_lib, used, spec, u, X, y, G, 6, setting)
            assert same_bits(b, c), setting
            assert np.array_equal(b["idx"], BO.reference("Matern52", 530, (20, 15), 6, *setting).picks)
    finally:
        fresh.close()
        used.close()


@pytest.mark.parametrize("setting", BO.SETTINGS, ids=[s[0] + "-%g-%g" % s[1:3] for s in BO.SETTINGS])
def test_mask(eng, setting):
    _lib, H = eng
    case = ("Matern52", 130, (13, 10), 8)
    kp, spec, u, X, y, G = IO.case(*case[:3])
    M = G.shape[0]
    free = BO.reference(*case, *setting)
    # the first three unmasked picks are excluded together with the last point of the grid: never picked, NaN in every
    # round, and the picks are the oracle's with that mask
    gone = sorted(set(free.picks[:3].tolist()) | {M - 1})
    mask = np.ones(M)
    mask[gone] = np.nan
    ref = BO.scheme(kp, X, y, G, 8, *setting, mask=mask)
    assert ref.gaps.min() >= 1e-7
    got = believer_abi(_lib, H, spec, u, X, y, G, 8, setting, mask=mask)
    check_against("mask without %s" % gone, got, ref, 8, M)
    assert not set(got["idx"].tolist()) & set(gone) and np.isnan(got["maps"][:, gone]).all()
    # the mask excludes candidates only: the entries it leaves have the bits of the unmasked round 0
    nomask = believer_abi(_lib, H, spec, u, X, y, G, 1, setting)
    keep = ~np.isnan(mask)
    assert np.array_equal(got["maps"][0][keep], nomask["maps"][0][keep])
    # three live candidates, six picks asked for
    few = np.full(M, np.nan)
    few[[4, 77, 129]] = 1.0
    ref = BO.scheme(kp, X, y, G, 6, *setting, mask=few)
    assert ref.gaps.min() >= 1e-7
    got = believer_abi(_lib, H, spec, u, X, y, G, 6, setting, mask=few)
    check_against("3 live candidates, q = 6", got, ref, 6, M, after_ref=BO.refit_variance(kp, X, G, ref.picks))
    assert got["count"][0] == 3 and sorted(got["idx"][:3].tolist()) == [4, 77, 129]
    assert np.all(got["idx"][3:] == -1) and np.isnan(got["val"][3:]).all() and np.isnan(got["maps"][3:]).all()
    # nothing live at all
    none = believer_abi(_lib, H, spec, u, X, y, G, 2, setting, mask=np.full(M, np.nan))
    assert none["count"][0] == 0 and np.all(none["idx"] == -1) and np.isnan(none["val"]).all() and np.isnan(none["maps"]).all()
    assert np.array_equal(none["sd_after"], none["sd"])


def test_refusals_of_the_entry(ensure_built):
    from gpim_amd import _lib
    kp, spec, u, X, y, G = IO.case("Matern52", 40, (6, 5))
    M, m = G.shape[0], spec.struct()
    Xd, yd, ud, Gd = X.cuda().contiguous(), y.cuda().contiguous(), u.cuda(), G.cuda().contiguous()
    idx = torch.zeros(M + 1, dtype=torch.int64, device="cuda")
    val, mean, sd = (torch.zeros(M + 1, dtype=torch.float64, device="cuda") for _ in range(3))
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    H, H32 = _lib.Handle(), _lib.Handle(precision="single")

    def call(handle=None, q=2, kind=1, Xp=Xd, Xobs=Xd, Mobs=X.shape[0], idx_=idx, val_=val, cnt_=cnt, mean_=mean, sd_=sd):
        handle = handle or H
        return handle.lib.gpimhip_acquire_batch(handle.h, ctypes.byref(m), _lib.ptr(Xp), _lib.ptr(yd), X.shape[0], _lib.ptr(ud),
                                                _lib.ptr(Gd), M, _lib.ptr(Xobs), Mobs, kind, 0.0, 0.01, None, q,
                                                _lib.ptr(mean_), _lib.ptr(sd_), None, None, _lib.ptr(idx_), _lib.ptr(val_),
                                                _lib.ptr(cnt_))
    try:
        assert call() == _lib.OK and cnt.item() == 2
        good = idx[:2].clone()
        for kw, word in ((dict(handle=H32), "double-precision"), (dict(q=0), "q = 0"), (dict(q=M + 1), "q = %d" % (M + 1)),
                         (dict(kind=3), "kind = 3"), (dict(kind=-1), "kind = -1"), (dict(Xobs=None), "Xobs"),
                         (dict(Mobs=0), "Xobs"), (dict(idx_=None), "idx_out"), (dict(val_=None), "idx_out"),
                         (dict(cnt_=None), "idx_out"), (dict(mean_=None), "idx_out"), (dict(sd_=None), "idx_out"),
                         (dict(Xp=None), "null")):
            bytes0 = H.lib.gpimhip_workspace_bytes(H.h)
            assert call(**kw) == _lib.E_BADARG, kw
            err = (kw.get("handle") or H).lib.gpimhip_last_error().decode()
            assert err.startswith("gpimhip_acquire_batch") and word in err, (kw, err)
            assert H.lib.gpimhip_workspace_bytes(H.h) == bytes0
        # CB needs no observed rows
        assert call(kind=0, Xobs=None, Mobs=0) == _lib.OK
        twoc = (ctypes.c_double * 4)(0, 0, 0, 0)
        assert H.lib.gpimhip_set_reflection(H.h, 1, twoc, None, X.shape[0], 0) == _lib.OK
        assert call() == _lib.E_BADARG and "reflection" in H.lib.gpimhip_last_error().decode()
        assert H.lib.gpimhip_set_reflection(H.h, 0, twoc, None, 0, 0) == _lib.OK
        idx.zero_()
        assert call() == _lib.OK and torch.equal(idx[:2], good)
        # q = M: every candidate, each once
        assert call(q=M) == _lib.OK and cnt.item() == M and sorted(idx[:M].tolist()) == list(range(M))
        # the entry's buffers are counted and released with the rest: W, the partial sums, v, the columns, live, incumbents
        b1 = H.lib.gpimhip_workspace_bytes(H.h)
        assert H.lib.gpimhip_set_precision(H.h, 32) == 0
        assert H.lib.gpimhip_workspace_bytes(H.h) <= b1 - 8 * (128 * 144 + 128 + 2 * M + M * 128 + M + M + 1)
    finally:
        H.close()
        H32.close()


# ------------------------------------------------------------------------------------------ Python surface
@pytest.fixture(scope="module")
def fitted(ensure_built):
    """the trained 16 x 16 model of tests/test_gpu_ivr.py's surface tests"""
    import gpim_amd
    R, _ = image16()
    r = gpim_amd.reconstructor(gpim_amd.utils.get_sparse_grid(R), R, gpim_amd.utils.get_full_grid(R), kernel="Matern52",
                               lengthscale=[[1., 1.], [8., 8.]], learning_rate=0.1, iterations=20, verbose=0)
    r.train()
    return gpim_amd, r, R


def host_scheme(sm, X_full, q, acqf, p0=0.0, p1=1.0, xi=0.01, mask=None):
    """the oracle's believer batch at the surrogate's current hyper-parameters and training data, flat over the grid"""
    spec = sm._spec
    kp = IO.kp_from_u(spec.kernel_type, spec.dim, [spec.ls_lo.tolist(), spec.ls_hi.tolist()], sm._u)
    G = torch.from_numpy(np.asarray(X_full, dtype=np.float64).reshape(spec.dim, -1).T.copy())
    return BO.scheme(kp, sm._Xd.cpu(), sm._yd.cpu(), G, q, acqf, p0, p1, xi, None if mask is None else np.ravel(mask),
                     jitter=spec.jitter)


def check_surface(tag, points, vals, maps, ref, shape):
    top = np.nanmax(np.abs(ref.maps[0]))
    n = len(ref.picks)
    want = [tuple(int(v) for v in np.unravel_index(p, shape)) for p in ref.picks]
    gap = np.nanmax(np.abs(maps["acq"].reshape(len(maps["acq"]), -1)[:n] - ref.maps))
    print("%s: points %s (oracle %s), smallest oracle gap %.2e, maps: max |gpu - ref| %.2e of max |map 0|, vals: %.2e of it"
          % (tag, points, want, ref.gaps.min(), gap / top, np.abs(vals - ref.vals).max() / top))
    assert ref.gaps.min() >= 1e-7           # (the condition of the pick comparison, as in tests/test_believer_host.py)
    assert points == want
    assert gap <= BAR * top and np.abs(vals - ref.vals).max() <= BAR * top


def test_reconstructor_acq_batch(fitted):
    gpim_amd, r, R = fitted
    Xf = gpim_amd.utils.get_full_grid(R)
    points, vals, maps = r.acq_batch(5, "ei")
    assert len(points) == 5 and all(isinstance(p, tuple) and len(p) == 2 for p in points) and len(set(points)) == 5
    assert isinstance(vals, np.ndarray) and vals.shape == (5,) and vals.dtype == np.float64
    assert maps["acq"].shape == (5, 16, 16) and maps["acq"].dtype == np.float64
    assert maps["mean"].shape == maps["sd"].shape == maps["sd_after"].shape == (16, 16)
    assert (maps["sd_after"] <= maps["sd"]).all() and np.isfinite(maps["sd_after"]).all()
    pm, psd = r.predict(verbose=0)
    assert np.abs(maps["mean"] - pm).max() <= 1e-10 and np.abs(maps["sd"] ** 2 - psd ** 2).max() <= 1e-10
    check_surface("acq_batch(5, 'ei') 16x16", points, vals, maps, host_scheme(r, Xf, 5, "ei"), (16, 16))
    mask = np.ones((16, 16))
    mask[:, :3] = np.nan
    pw, vw, mw = r.acq_batch(5, "ei", mask=mask)
    check_surface("acq_batch(5, 'ei') 16x16, mask", pw, vw, mw, host_scheme(r, Xf, 5, "ei", mask=mask), (16, 16))
    assert all(p[1] >= 3 for p in pw) and np.isnan(mw["acq"][:, :, :3]).all()
    Xc = Xf[:, 2:9, 3:8]
    pc, vc, mc = r.acq_batch(5, "ei", Xtest=Xc)
    assert mc["acq"].shape == (5, 7, 5)
    check_surface("acq_batch(5, 'ei') 7x5 crop", pc, vc, mc, host_scheme(r, Xc, 5, "ei"), (7, 5))
    pb, vb, mb = r.acq_batch(5, "cb", alpha=1, beta=2, Xtest=Xf)
    check_surface("acq_batch(5, 'cb', 1, 2) 16x16", pb, vb, mb, host_scheme(r, Xf, 5, "cb", 1.0, 2.0), (16, 16))
    # more picks than candidates: every candidate once
    pa, va, ma = r.acq_batch(40, "poi", Xtest=Xc)
    assert len(pa) == 35 and len(set(pa)) == 35 and ma["acq"].shape == (35, 7, 5)
    r.predict(Xf, verbose=0)
    for bad in (dict(n_points=0), dict(n_points=-2), dict(n_points=3, acquisition_function="ivr"),
                dict(n_points=3, mask=np.ones((16, 15))), dict(n_points=3, mask=np.ones(256)),
                dict(n_points=3, mask=np.zeros((16, 16)))):
        with pytest.raises(ValueError):
            r.acq_batch(**bad)
    Xnan = Xf.astype(np.float64)
    Xnan[:, 3, 4] = np.nan
    with pytest.raises(ValueError):
        r.acq_batch(3, Xtest=Xnan)


def test_refusals_of_the_surface(fitted, tmp_path):
    gpim_amd, r, R = fitted
    Xs, Xf = gpim_amd.utils.get_sparse_grid(R), gpim_amd.utils.get_full_grid(R)
    _, full = image16()
    models = [(gpim_amd.reconstructor(Xs, R, Xf, precision="single", iterations=1, verbose=0), "single precision"),
              (gpim_amd.reconstructor(Xs, R, Xf, sparse=True, indpoints=20, iterations=1, verbose=0), "inducing points"),
              (gpim_amd.reconstructor(Xf, full, Xf, structured=True, iterations=1, verbose=0), "not block-structured")]
    for model, why in models:
        with pytest.raises(NotImplementedError, match=why):
            model.acq_batch(3)
    with pytest.raises(NotImplementedError):
        gpim_amd.skreconstructor(Xf, full, Xf, kernel="Matern52", iterations=1, verbose=0).acq_batch(3)
    kw = dict(exploration_steps=1, gp_iterations=1, verbose=0, filename=str(tmp_path / "bo"))
    for af in ("cb", "ei", "poi"):
        with pytest.raises(ValueError, match="acq_batch"):
            gpim_amd.boptimizer(Xs, R.copy(), Xf, lambda idx: 0.0, acquisition_function=af, batch_update=True, acq_batch="x", **kw)
    for extra in (dict(precision="single"), dict(sparse=True, indpoints=20), dict(shard_candidates=True)):
        with pytest.raises(NotImplementedError):
            gpim_amd.boptimizer(Xs, R.copy(), Xf, lambda idx: 0.0, acquisition_function="ei", batch_update=True,
                                acq_batch="believer", **dict(kw, **extra))
    # the option belongs to 'cb' / 'ei' / 'poi' alone, as ts_batch to 'ts'
    gpim_amd.boptimizer(Xs, R.copy(), Xf, lambda idx: 0.0, **dict(kw, acquisition_function="ivr", acq_batch="x"))
    with pytest.raises(ValueError):
        gpim_amd.acqfunc.believer_on_device(r, "ei", r._Xtest_d, 0)
    with pytest.raises(ValueError):
        gpim_amd.acqfunc.believer_on_device(r, "ei", r._Xtest_d, 257)
    with pytest.raises(ValueError):
        gpim_amd.acqfunc.believer_on_device(r, "ts", r._Xtest_d, 3)


def believer_campaign(gpim_amd, tmp_path, af, **kw):
    """boptimizer(af, batch_update=True) on the 25 x 25 problem of config C4 (four scattered seed points, three steps);
    returns the optimiser and, per step, the oracle's believer batch at that step's hyper-parameters and training data"""
    from problems import notebook_problem
    trial_func, Z = notebook_problem(4)
    bo = gpim_amd.boptimizer(gpim_amd.utils.get_sparse_grid(Z), Z.copy(), gpim_amd.utils.get_full_grid(Z), trial_func,
                             acquisition_function=af, exploration_steps=3, gp_iterations=50, verbose=0, batch_update=True,
                             filename=str(tmp_path / "bo"), **kw)
    refs, inner = [], bo.next_point

    def spy():
        refs.append(host_scheme(bo.surrogate_model, bo.X_full, bo.batch_out_max, af, bo.alpha, bo.beta, bo.xi, kw.get("mask")))
        return inner()
    bo.next_point = spy
    return bo, refs


@pytest.mark.parametrize("af,masked", [("ei", False), ("cb", False), ("ei", True)], ids=["ei", "cb", "ei-mask"])
def test_boptimizer_believer_batches(ensure_built, tmp_path, af, masked):
    import gpim_amd
    kw = {}
    if masked:
        mask = np.full((25, 25), np.nan)
        mask[5:20, 5:20] = 1.0
        kw = dict(mask=mask)
    bo, refs = believer_campaign(gpim_amd, tmp_path, af, acq_batch="believer", batch_out_max=4, **kw)
    bo.run()
    assert len(refs) == 3 and len(bo.indices_all) == 12 and len(bo.vals_all) == 12 and len(bo.gp_predictions) == 3
    for e, ref in enumerate(refs):
        got = [tuple(int(v) for v in i) for i in bo.indices_all[4 * e:4 * e + 4]]
        want = [tuple(int(v) for v in np.unravel_index(p, (25, 25))) for p in ref.picks]
        vals = np.array(bo.vals_all[4 * e:4 * e + 4])
        top = np.nanmax(np.abs(ref.maps[0]))
        print("step %d: batch %s, oracle %s, smallest oracle gap %.2e, vals: max |gpu - ref| %.2e of max |map 0|"
              % (e, got, want, ref.gaps.min(), np.abs(vals - ref.vals).max() / top))
        assert ref.gaps.min() >= 1e-7       # (the condition of the pick comparison)
        assert got == want and len(set(got)) == 4
        assert np.abs(vals - ref.vals).max() <= BAR * top
        if masked:
            assert all(kw["mask"][p] == 1.0 for p in got)
    for mean, sd in bo.gp_predictions:
        assert mean.shape == sd.shape == (25, 25) and np.isfinite(mean).all() and (sd > 0).all()


@pytest.mark.parametrize("af", ["cb", "ei", "poi"])
def test_boptimizer_thin_is_the_default(ensure_built, tmp_path, af):
    """acq_batch='thin' and no option at all return the batch of the ranked and thinned single map
    (acquisition_on_device, the device ranking, update_points), value for value"""
    import gpim_amd
    from gpim_amd import acqfunc
    out = []
    for kw in ({}, dict(acq_batch="thin")):
        bo, _ = believer_campaign(gpim_amd, tmp_path, af, batch_size=50, batch_out_max=4, **kw)
        bo.surrogate_model.train()
        np.random.seed(11)
        vals, inds = bo.__class__.next_point(bo)
        assert len(vals) == len(inds) == 4
        sm = bo.surrogate_model
        p0, p1 = (bo.alpha, bo.beta) if af == "cb" else (0.0, 0.0)
        acq_d, _, _ = acqfunc.acquisition_on_device(sm, af, bo.X_full, bo.X_sparse, p0, p1, bo.xi, Xf_d=bo._Xfull_d,
                                                    Xobs_d=bo._observed_rows_d())
        rv, ri = bo._rank_device(acq_d, (25, 25), masked=True)
        np.random.seed(11)
        pv, pi = bo.update_points(rv, ri, sm.model.kernel.lengthscale.mean().item())
        assert vals == pv and inds == pi
        out.append((vals, inds))
    assert out[0] == out[1]
