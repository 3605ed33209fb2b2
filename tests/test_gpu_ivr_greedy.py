"""
The greedy batch of integrated variance reduction on the MI355X (gpimhip_ivr_greedy, reconstructor.ivr_batch,
boptimizer(ivr_batch='greedy')) against the float64 scheme of tests/ivr_greedy_oracle.py (`greedy`: posterior_cov, then map /
arg-max / C -= g g^T in numpy), which tests/test_ivr_greedy_host.py holds to M-point refits at 1e-12.

Bars, per case:
  picks       equal to the oracle's, exactly: the host test shows every round's best value leading the second best by >= 1e-6
              relative (smallest: 8.4e-5), four orders above the bar on the maps, so an engine inside that bar cannot flip one
  maps, gains max |gpu - ref| <= 1e-10 max(round-0 reference map), at the entries that are not NaN -- DESIGN.md section 26's bar
  NaN         in row r exactly at the picks of the rounds before r
  sd_after^2  against predict's variance of the dense oracle refitted with the whole batch: <= 1e-10 relative, the project's
              bar for a dense double variance
The shapes are the smallest that reach each path of the fused pass (tests/ivr_greedy_oracle.py: CASES).  Every test prints the
distances it measured before it asserts.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ivr_oracle as IO
import ivr_greedy_oracle as GO
from test_gpu_ivr import ivr_abi, image16
from test_ivr_greedy_host import ident

BAR = 1e-10
NAMES = ("idx", "gain", "count", "maps", "mean", "sd", "sd_after")


@pytest.fixture(scope="module")
def eng(ensure_built):
    from gpim_amd import _lib
    H = _lib.Handle()
    yield _lib, H
    H.close()


def greedy_abi(_lib, H, spec, u, X, y, G, q, w=None, mask=None, want=True):
    """dict of numpy arrays (NAMES) of gpimhip_ivr_greedy on the handle H; maps, mean, sd, sd_after None without `want`"""
    M = G.shape[0]
    m = spec.struct()
    Xd, yd, ud, Gd = X.cuda().contiguous(), y.cuda().contiguous(), u.cuda(), G.cuda().contiguous()
    wd = None if w is None else torch.as_tensor(w, dtype=torch.float64).cuda().contiguous()
    md = None if mask is None else torch.as_tensor(mask, dtype=torch.float64).cuda().contiguous()
    # three sentinels behind every output
    f = lambda n: torch.full((n + 3,), -7.0, dtype=torch.float64, device="cuda")
    gain, maps, mean, sd, after = f(q), f(q * M), f(M), f(M), f(M)
    idx = torch.full((q + 3,), -7, dtype=torch.int64, device="cuda")
    count = torch.full((1 + 3,), -7, dtype=torch.int64, device="cuda")
    opt = lambda t: _lib.ptr(t) if want else None
    _lib.check(H.lib.gpimhip_ivr_greedy(H.h, ctypes.byref(m), _lib.ptr(Xd), _lib.ptr(yd), X.shape[0], _lib.ptr(ud), _lib.ptr(Gd),
                                        M, _lib.ptr(wd), _lib.ptr(md), q, opt(mean), opt(sd), opt(maps), opt(after),
                                        _lib.ptr(idx), _lib.ptr(gain), _lib.ptr(count)))
    out = {}
    for name, t, n in (("idx", idx, q), ("gain", gain, q), ("count", count, 1), ("maps", maps, q * M), ("mean", mean, M),
                       ("sd", sd, M), ("sd_after", after, M)):
        h = t.cpu().numpy()
        assert np.all(h[n:] == -7), name
        out[name] = h[:n] if want or name in ("idx", "gain", "count") else None
    if want:
        out["maps"] = out["maps"].reshape(q, M)
    return out


def same_bits(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k], equal_nan=True) for k in NAMES)


def check_against(tag, got, ref, q, M, after_ref=None):
    """the bars of the module docstring, for the rounds the oracle made"""
    n = len(ref.picks)
    top = np.nanmax(ref.maps[0])
    on = ~np.isnan(ref.maps)
    gap = np.abs(got["maps"][:n] - ref.maps)[on].max()
    ggap = np.abs(got["gain"][:n] - ref.gains).max()
    print("%s: picks %s (oracle %s), max a %.4f, maps: max |gpu - ref| %.2e = %.2e of max a, gains: %.2e = %.2e of max a; "
          "smallest oracle gap %.2e" % (tag, got["idx"].tolist(), ref.picks.tolist(), top, gap, gap / top, ggap, ggap / top,
                                        ref.gaps.min()))
    assert got["count"][0] == n
    assert np.array_equal(got["idx"][:n], ref.picks) and np.all(got["idx"][n:] == -1) and np.isnan(got["gain"][n:]).all()
    assert np.array_equal(np.isnan(got["maps"][:n]), ~on) and np.isnan(got["maps"][n:]).all()
    assert gap <= BAR * top and ggap <= BAR * top
    assert np.isfinite(got["mean"]).all() and np.isfinite(got["sd"]).all() and np.isfinite(got["sd_after"]).all()
    if after_ref is not None:
        rel = np.abs(got["sd_after"] ** 2 / after_ref - 1.0).max()
        print("    sd_after^2 against the refit's predict: max rel %.2e" % rel)
        assert rel <= BAR


@pytest.mark.parametrize("kind,N,shape,q,wseed", GO.CASES, ids=[ident(c) for c in GO.CASES])
def test_against_oracle(eng, kind, N, shape, q, wseed):
    _lib, H = eng
    kp, spec, u, X, y, G = IO.case(kind, N, shape)
    M = G.shape[0]
    assert len(X) == N
    w = None if wseed is None else IO.weights(M, wseed)
    ref = GO.reference(kind, N, shape, q, wseed)
    assert len(ref.picks) == q
    got = greedy_abi(_lib, H, spec, u, X, y, G, q, w=w)
    check_against("%s N=%d grid %s q=%d weights %s" % (kind, N, shape, q, wseed), got, ref, q, M,
                  after_ref=GO.refit_variance(kp, X, G, ref.picks))
    # every pick lowers every variance
    assert (got["sd_after"] <= got["sd"]).all()


def test_one_pick_is_ivr_exact(eng):
    """q = 1: map, mean and sd have the bits of gpimhip_ivr_exact on the same handle, the index is gpimhip_topk's first, and
    sd_after is the refit's; with weights and a mask"""
    _lib, H = eng
    kind, N, shape = "Matern52", 300, (25, 25)
    kp, spec, u, X, y, G = IO.case(kind, N, shape)
    M = G.shape[0]
    for w, mask in ((None, None), (IO.weights(M, 7), np.where(np.arange(M) % 7 == 3, np.nan, 1.0))):
        a, mean, sd = ivr_abi(_lib, H, spec, u, X, y, G, w=w, mask=mask)
        got = greedy_abi(_lib, H, spec, u, X, y, G, 1, w=w, mask=mask)
        assert np.array_equal(got["maps"][0], a, equal_nan=True)
        assert np.array_equal(got["mean"], mean) and np.array_equal(got["sd"], sd)
        ad = torch.from_numpy(a).cuda()
        vals, idx, cnt = (torch.zeros(1, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"),
                          torch.zeros(1, dtype=torch.int64, device="cuda"))
        _lib.check(H.lib.gpimhip_topk(H.h, _lib.ptr(ad), M, 1, 0, _lib.ptr(vals), _lib.ptr(idx), _lib.ptr(cnt)))
        print("q = 1: pick %d, topk %d, gain %.12g" % (got["idx"][0], idx.item(), got["gain"][0]))
        assert got["count"][0] == 1 and got["idx"][0] == idx.item() and got["gain"][0] == vals.item() == np.nanmax(a)
        rel = np.abs(got["sd_after"] ** 2 / GO.refit_variance(kp, X, G, got["idx"]) - 1.0).max()
        print("    sd_after^2 against the refit's predict: max rel %.2e" % rel)
        assert rel <= BAR
        # the outputs that are not wanted change nothing
        lean = greedy_abi(_lib, H, spec, u, X, y, G, 1, w=w, mask=mask, want=False)
        assert lean["idx"][0] == got["idx"][0] and lean["gain"][0] == got["gain"][0] and lean["maps"] is None


def test_two_calls_same_bits_and_covariance_rebuilt(eng):
    """Two calls give identical bits in every output, with and without the optional outputs; after a greedy call (which
    leaves a downdated C behind) gpimhip_ivr_exact on that handle returns the bits of a fresh handle."""
    _lib, H = eng
    kp, spec, u, X, y, G = IO.case("Matern52", 300, (25, 25))
    w = IO.weights(G.shape[0], 7)
    a = greedy_abi(_lib, H, spec, u, X, y, G, 8, w=w)
    b = greedy_abi(_lib, H, spec, u, X, y, G, 8, w=w)
    assert same_bits(a, b)
    c = greedy_abi(_lib, H, spec, u, X, y, G, 8, w=w, want=False)
    assert np.array_equal(c["idx"], a["idx"]) and np.array_equal(c["gain"], a["gain"]) and c["count"][0] == 8
    fresh = _lib.Handle()
    try:
        e0 = ivr_abi(_lib, fresh, spec, u, X, y, G, w=w)
    finally:
        fresh.close()
    e1 = ivr_abi(_lib, H, spec, u, X, y, G, w=w)
    assert all(np.array_equal(p, q) for p, q in zip(e0, e1))
    assert np.array_equal(a["maps"][0], e0[0])


def test_ragged_block_and_stale_padding(eng):
    """DESIGN.md section 26's stale-W case through the new entry: a handle that fitted N = 600 (every row of the workspace
    written) and ran a greedy batch of that order returns at N = 530 (np = 640, 18 valid rows in the last block) the bits
    of a fresh handle."""
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
        greedy_abi(_lib, used, s6, u6.cpu(), X6, y6, G, 6)
        b = greedy_abi(_lib, fresh, spec, u, X, y, G, 6)
        c = greedy_abi(_lib, used, spec, u, X, y, G, 6)
    finally:
        fresh.close()
        used.close()
    assert same_bits(b, c)
    assert np.array_equal(b["idx"], GO.reference("Matern52", 530, (20, 15), 6).picks)


def test_mask(eng):
    _lib, H = eng
    kind, N, shape = "Matern52", 130, (13, 10)
    kp, spec, u, X, y, G = IO.case(kind, N, shape)
    M = G.shape[0]
    free = GO.reference(kind, N, shape, 8)
    # the first three unmasked picks are excluded (one of them in the second tile or not, as the problem has it) together
    # with the last point of the grid: never picked, NaN in every round, and the picks are the oracle's with that mask
    gone = sorted(set(free.picks[:3].tolist()) | {M - 1})
    mask = np.ones(M)
    mask[gone] = np.nan
    ref = GO.greedy(kp, X, G, 8, mask=mask)
    assert ref.gaps.min() >= 1e-6
    got = greedy_abi(_lib, H, spec, u, X, y, G, 8, mask=mask)
    check_against("mask without %s" % gone, got, ref, 8, M)
    assert not set(got["idx"].tolist()) & set(gone) and np.isnan(got["maps"][:, gone]).all()
    # the mask excludes candidates only: the entries it leaves have the bits of the unmasked round 0
    nomask = greedy_abi(_lib, H, spec, u, X, y, G, 1)
    keep = ~np.isnan(mask)
    assert np.array_equal(got["maps"][0][keep], nomask["maps"][0][keep])
    # three live candidates, six picks asked for
    few = np.full(M, np.nan)
    few[[4, 77, 129]] = 1.0
    ref = GO.greedy(kp, X, G, 6, mask=few)
    got = greedy_abi(_lib, H, spec, u, X, y, G, 6, mask=few)
    check_against("3 live candidates, q = 6", got, ref, 6, M, after_ref=GO.refit_variance(kp, X, G, ref.picks))
    assert got["count"][0] == 3 and sorted(got["idx"][:3].tolist()) == [4, 77, 129]
    assert np.all(got["idx"][3:] == -1) and np.isnan(got["gain"][3:]).all()
    # nothing live at all
    none = greedy_abi(_lib, H, spec, u, X, y, G, 2, mask=np.full(M, np.nan))
    assert none["count"][0] == 0 and np.all(none["idx"] == -1) and np.isnan(none["gain"]).all() and np.isnan(none["maps"]).all()
    assert np.array_equal(none["sd_after"], none["sd"])


def test_ties_go_to_the_larger_index(eng):
    """weights of zero: every value is 0 in every round, the picks are the largest live flat indices, as gpimhip_topk ranks"""
    _lib, H = eng
    kp, spec, u, X, y, G = IO.case("Matern52", 130, (13, 10))
    got = greedy_abi(_lib, H, spec, u, X, y, G, 3, w=np.zeros(130))
    assert got["idx"].tolist() == [129, 128, 127] and (got["gain"] == 0.0).all() and got["count"][0] == 3


def test_refusals_of_the_entry(ensure_built):
    from gpim_amd import _lib
    kp, spec, u, X, y, G = IO.case("Matern52", 40, (6, 5))
    M, m = G.shape[0], spec.struct()
    Xd, yd, ud, Gd = X.cuda().contiguous(), y.cuda().contiguous(), u.cuda(), G.cuda().contiguous()
    idx = torch.zeros(M + 1, dtype=torch.int64, device="cuda")
    gain = torch.zeros(M + 1, dtype=torch.float64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    H, H32 = _lib.Handle(), _lib.Handle(precision="single")

    def call(handle=None, q=2, Xp=Xd, idx_=idx, gain_=gain, cnt_=cnt):
        handle = handle or H
        return handle.lib.gpimhip_ivr_greedy(handle.h, ctypes.byref(m), _lib.ptr(Xp), _lib.ptr(yd), X.shape[0], _lib.ptr(ud),
                                             _lib.ptr(Gd), M, None, None, q, None, None, None, None, _lib.ptr(idx_),
                                             _lib.ptr(gain_), _lib.ptr(cnt_))
    try:
        assert call() == _lib.OK and cnt.item() == 2
        good = idx[:2].clone()
        for kw, word in ((dict(handle=H32), "double-precision"), (dict(q=0), "q = 0"), (dict(q=M + 1), "q = %d" % (M + 1)),
                         (dict(idx_=None), "idx_out"), (dict(gain_=None), "idx_out"), (dict(cnt_=None), "idx_out"),
                         (dict(Xp=None), "null")):
            bytes0 = H.lib.gpimhip_workspace_bytes(H.h)
            assert call(**kw) == _lib.E_BADARG, kw
            err = (kw.get("handle") or H).lib.gpimhip_last_error().decode()
            assert err.startswith("gpimhip_ivr_greedy") and word in err, (kw, err)
            assert H.lib.gpimhip_workspace_bytes(H.h) == bytes0
        twoc = (ctypes.c_double * 4)(0, 0, 0, 0)
        assert H.lib.gpimhip_set_reflection(H.h, 1, twoc, None, X.shape[0], 0) == _lib.OK
        assert call() == _lib.E_BADARG and "reflection" in H.lib.gpimhip_last_error().decode()
        assert H.lib.gpimhip_set_reflection(H.h, 0, twoc, None, 0, 0) == _lib.OK
        idx.zero_()
        assert call() == _lib.OK and torch.equal(idx[:2], good)
        # q = M: every candidate, each once
        assert call(q=M) == _lib.OK and cnt.item() == M and sorted(idx[:M].tolist()) == list(range(M))
        # the O(M) buffers are counted and released with the rest
        b1 = H.lib.gpimhip_workspace_bytes(H.h)
        assert H.lib.gpimhip_set_precision(H.h, 32) == 0
        assert H.lib.gpimhip_workspace_bytes(H.h) <= b1 - 8 * (128 * 144 * 2 + 128 + 128 + M + M)
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


def host_greedy(sm, X_full, q, w=None, mask=None):
    """the oracle's greedy batch at the surrogate's current hyper-parameters and training rows, flat over the grid"""
    spec = sm._spec
    kp = IO.kp_from_u(spec.kernel_type, spec.dim, [spec.ls_lo.tolist(), spec.ls_hi.tolist()], sm._u)
    G = torch.from_numpy(np.asarray(X_full, dtype=np.float64).reshape(spec.dim, -1).T.copy())
    return GO.greedy(kp, sm._Xd.cpu(), G, q, None if w is None else np.ravel(w), None if mask is None else np.ravel(mask),
                     jitter=spec.jitter)


def check_surface(tag, points, gains, maps, ref, shape):
    top = np.nanmax(ref.maps[0])
    n = len(ref.picks)
    want = [tuple(int(v) for v in np.unravel_index(p, shape)) for p in ref.picks]
    gap = np.nanmax(np.abs(maps["ivr"].reshape(len(maps["ivr"]), -1)[:n] - ref.maps))
    print("%s: points %s (oracle %s), smallest oracle gap %.2e, maps: max |gpu - ref| %.2e of max a, gains: %.2e of max a"
          % (tag, points, want, ref.gaps.min(), gap / top, np.abs(gains - ref.gains).max() / top))
    assert ref.gaps.min() >= 1e-6           # (the condition of the pick comparison, as in tests/test_ivr_greedy_host.py)
    assert points == want
    assert gap <= BAR * top and np.abs(gains - ref.gains).max() <= BAR * top


def test_reconstructor_ivr_batch(fitted):
    gpim_amd, r, R = fitted
    Xf = gpim_amd.utils.get_full_grid(R)
    a0 = r.ivr()[0]
    points, gains, maps = r.ivr_batch(5)
    assert len(points) == 5 and all(isinstance(p, tuple) and len(p) == 2 for p in points) and len(set(points)) == 5
    assert isinstance(gains, np.ndarray) and gains.shape == (5,) and gains.dtype == np.float64
    assert maps["ivr"].shape == (5, 16, 16) and maps["ivr"].dtype == np.float64
    assert maps["mean"].shape == maps["sd"].shape == maps["sd_after"].shape == (16, 16)
    assert np.array_equal(maps["ivr"][0], a0)
    assert (maps["sd_after"] <= maps["sd"]).all() and np.isfinite(maps["sd_after"]).all()
    pm, psd = r.predict(verbose=0)
    assert np.abs(maps["mean"] - pm).max() <= 1e-10 and np.abs(maps["sd"] ** 2 - psd ** 2).max() <= 1e-10
    check_surface("ivr_batch(5) 16x16", points, gains, maps, host_greedy(r, Xf, 5), (16, 16))
    w = IO.weights(256, 3).reshape(16, 16)
    mask = np.ones((16, 16))
    mask[:, :3] = np.nan
    pw, gw, mw = r.ivr_batch(5, weights=w, mask=mask)
    check_surface("ivr_batch(5) 16x16, weights and mask", pw, gw, mw, host_greedy(r, Xf, 5, w, mask), (16, 16))
    assert all(p[1] >= 3 for p in pw) and np.isnan(mw["ivr"][:, :, :3]).all()
    Xc = Xf[:, 2:9, 3:8]
    pc, gc, mc = r.ivr_batch(5, Xtest=Xc)
    assert mc["ivr"].shape == (5, 7, 5) and np.array_equal(mc["ivr"][0], r.ivr(Xtest=Xc)[0])
    check_surface("ivr_batch(5) 7x5 crop", pc, gc, mc, host_greedy(r, Xc, 5), (7, 5))
    # more picks than candidates: every candidate once
    pa, ga, ma = r.ivr_batch(40, Xtest=Xc)
    assert len(pa) == 35 and len(set(pa)) == 35 and ma["ivr"].shape == (35, 7, 5)
    r.ivr(Xtest=Xf)
    for bad in (dict(n_points=0), dict(n_points=-2), dict(n_points=3, weights=-np.ones((16, 16))),
                dict(n_points=3, weights=np.ones((16, 15))), dict(n_points=3, mask=np.ones((16, 15))),
                dict(n_points=3, mask=np.ones(256)), dict(n_points=3, mask=np.zeros((16, 16)))):
        with pytest.raises(ValueError):
            r.ivr_batch(**bad)
    Xnan = Xf.astype(np.float64)
    Xnan[:, 3, 4] = np.nan
    with pytest.raises(ValueError):
        r.ivr_batch(3, Xtest=Xnan)


def test_refusals_of_the_surface(fitted, tmp_path):
    gpim_amd, r, R = fitted
    Xs, Xf = gpim_amd.utils.get_sparse_grid(R), gpim_amd.utils.get_full_grid(R)
    _, full = image16()
    models = [(gpim_amd.reconstructor(Xs, R, Xf, precision="single", iterations=1, verbose=0), "single precision"),
              (gpim_amd.reconstructor(Xs, R, Xf, sparse=True, indpoints=20, iterations=1, verbose=0), "inducing points"),
              (gpim_amd.reconstructor(Xf, full, Xf, structured=True, iterations=1, verbose=0), "not block-structured")]
    for model, why in models:
        with pytest.raises(NotImplementedError, match=why):
            model.ivr_batch(3)
    with pytest.raises(NotImplementedError):
        gpim_amd.skreconstructor(Xf, full, Xf, kernel="Matern52", iterations=1, verbose=0).ivr_batch(3)
    assert not hasattr(gpim_amd.vreconstructor, "ivr_batch")
    kw = dict(acquisition_function="ivr", exploration_steps=1, gp_iterations=1, verbose=0, filename=str(tmp_path / "bo"))
    with pytest.raises(ValueError, match="ivr_batch"):
        gpim_amd.boptimizer(Xs, R.copy(), Xf, lambda idx: 0.0, batch_update=True, ivr_batch="x", **kw)
    with pytest.raises(NotImplementedError):
        gpim_amd.boptimizer(Xs, R.copy(), Xf, lambda idx: 0.0, batch_update=True, ivr_batch="greedy", precision="single", **kw)
    # the option belongs to 'ivr' alone, as ts_batch to 'ts'
    gpim_amd.boptimizer(Xs, R.copy(), Xf, lambda idx: 0.0, **dict(kw, acquisition_function="cb", ivr_batch="x"))
    with pytest.raises(ValueError):
        gpim_amd.acqfunc.ivr_greedy_on_device(r, r._Xtest_d, 0)
    with pytest.raises(ValueError):
        gpim_amd.acqfunc.ivr_greedy_on_device(r, r._Xtest_d, 257)


def greedy_campaign(gpim_amd, tmp_path, **kw):
    """boptimizer('ivr', batch_update=True) on the 25 x 25 problem of config C4 (four scattered seed points, three steps);
    returns the optimiser and, per step, the oracle's greedy batch at that step's hyper-parameters and training rows"""
    from problems import notebook_problem
    trial_func, Z = notebook_problem(4)
    bo = gpim_amd.boptimizer(gpim_amd.utils.get_sparse_grid(Z), Z.copy(), gpim_amd.utils.get_full_grid(Z), trial_func,
                             acquisition_function="ivr", exploration_steps=3, gp_iterations=50, verbose=0, batch_update=True,
                             filename=str(tmp_path / "bo"), **kw)
    refs, inner = [], bo.next_point

    def spy():
        refs.append(host_greedy(bo.surrogate_model, bo.X_full, bo.batch_out_max, kw.get("ivr_weights"), kw.get("mask")))
        return inner()
    bo.next_point = spy
    return bo, refs


@pytest.mark.parametrize("masked", [False, True], ids=["free", "mask"])
def test_boptimizer_greedy_batches(ensure_built, tmp_path, masked):
    import gpim_amd
    kw = {}
    if masked:
        mask = np.full((25, 25), np.nan)
        mask[5:20, 5:20] = 1.0
        kw = dict(mask=mask, ivr_weights=IO.weights(625, 5).reshape(25, 25))
    bo, refs = greedy_campaign(gpim_amd, tmp_path, ivr_batch="greedy", batch_out_max=4, **kw)
    bo.run()
    assert len(refs) == 3 and len(bo.indices_all) == 12 and len(bo.vals_all) == 12 and len(bo.gp_predictions) == 3
    for e, ref in enumerate(refs):
        got = [tuple(int(v) for v in i) for i in bo.indices_all[4 * e:4 * e + 4]]
        want = [tuple(int(v) for v in np.unravel_index(p, (25, 25))) for p in ref.picks]
        vals = np.array(bo.vals_all[4 * e:4 * e + 4])
        top = np.nanmax(ref.maps[0])
        print("step %d: batch %s, oracle %s, smallest oracle gap %.2e, gains: max |gpu - ref| %.2e of max a"
              % (e, got, want, ref.gaps.min(), np.abs(vals - ref.gains).max() / top))
        assert ref.gaps.min() >= 1e-6       # (the condition of the pick comparison)
        assert got == want and len(set(got)) == 4
        assert np.abs(vals - ref.gains).max() <= BAR * top
        if masked:
            assert all(kw["mask"][p] == 1.0 for p in got)
    for mean, sd in bo.gp_predictions:
        assert mean.shape == sd.shape == (25, 25) and np.isfinite(mean).all() and (sd > 0).all()


def test_boptimizer_thin_is_the_default(ensure_built, tmp_path):
    """ivr_batch='thin' and no option at all return the batch of the ranked and thinned single map (ivr_on_device, the
    device ranking, update_points), value for value"""
    import gpim_amd
    from gpim_amd import acqfunc
    out = []
    for kw in ({}, dict(ivr_batch="thin")):
        bo, _ = greedy_campaign(gpim_amd, tmp_path, batch_size=50, batch_out_max=4, **kw)
        bo.surrogate_model.train()
        np.random.seed(11)
        vals, inds = bo.__class__.next_point(bo)
        assert len(vals) == len(inds) == 4
        sm = bo.surrogate_model
        acq_d, _, _ = acqfunc.ivr_on_device(sm, bo._Xfull_d)
        rv, ri = bo._rank_device(acq_d, (25, 25), masked=True)
        np.random.seed(11)
        pv, pi = bo.update_points(rv, ri, sm.model.kernel.lengthscale.mean().item())
        assert vals == pv and inds == pi
        out.append((vals, inds))
    assert out[0] == out[1]
