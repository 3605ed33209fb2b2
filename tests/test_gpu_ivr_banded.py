"""
Integrated variance reduction in bands on the MI355X (gpimhip_ivr_exact_banded, gpimhip_ivr_greedy_banded, the `band`
argument of reconstructor.ivr / ivr_batch, boptimizer(ivr_band=...)) against the float64 references of
tests/ivr_oracle.py (`closed`, `brute`) and tests/ivr_greedy_oracle.py (`greedy`), and against the stored entries.

Bars, the project's own (sections 26 / 27):
  maps, gains   max |gpu - ref| <= 1e-10 max(a_ref)
  mean          1e-10 absolute, sd^2 and sd_after^2 1e-10 relative (against the dense oracle's predict, refitted for sd_after)
  picks         the oracle's, exactly (tests/test_ivr_greedy_host.py: every best-to-second gap >= 8.4e-5)
  banded against stored (exact entry), two banded calls, band = 1 against band = 5: equal bits -- the kernel build computes an
                entry from its own (row, column) pair, the TN launch contracts every tile over the same k-range whatever
                workgroup shape the launch's tile count selects (the shapes split a tile in space, never in k), and every slot
                of the partial sums is written by the same tile's walk and added in the same order
Settings: noise_u = -3, jitter 1e-5, the candidates of ivr_oracle.grid.  Shapes: the smallest with several block columns, an
uneven last band, a last tile that is not full and a ragged last block of W.  Every test prints what it measured before it
asserts.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import gpim_oracle as O
import ivr_oracle as IO
import ivr_greedy_oracle as GO
from test_gpu_ivr import ivr_abi, image16, check, host_ivr, campaign, check_picks
from test_gpu_ivr_greedy import greedy_abi, same_bits, check_against, host_greedy, check_surface, greedy_campaign

BAR = 1e-10


@pytest.fixture(scope="module")
def eng(ensure_built):
    from gpim_amd import _lib
    H = _lib.Handle()
    yield _lib, H
    H.close()


def dev(t):
    return None if t is None else torch.as_tensor(t, dtype=torch.float64).cuda().contiguous()


def banded_abi(_lib, H, spec, u, X, y, G, band, w=None, mask=None, want_post=True):
    """(acq, mean, sd) numpy arrays of gpimhip_ivr_exact_banded on the handle H (mean, sd None without want_post)"""
    M = G.shape[0]
    m = spec.struct()
    Xd, yd, ud, Gd, wd, md = dev(X), dev(y), u.cuda(), dev(G), dev(w), dev(mask)
    # three sentinels behind every output: only M entries are written
    acq, mean, sd = (torch.full((M + 3,), -7.0, dtype=torch.float64, device="cuda") for _ in range(3))
    _lib.check(H.lib.gpimhip_ivr_exact_banded(H.h, ctypes.byref(m), _lib.ptr(Xd), _lib.ptr(yd), X.shape[0], _lib.ptr(ud),
                                              _lib.ptr(Gd), M, band, _lib.ptr(wd), _lib.ptr(md),
                                              _lib.ptr(mean) if want_post else None, _lib.ptr(sd) if want_post else None,
                                              _lib.ptr(acq)))
    out = [t.cpu().numpy() for t in (acq, mean, sd)]
    assert all(np.all(o[M:] == -7.0) for o in out)
    return out[0][:M], (out[1][:M] if want_post else None), (out[2][:M] if want_post else None)


def greedy_banded_abi(_lib, H, spec, u, X, y, G, q, band, w=None, mask=None, want=True):
    """dict of numpy arrays of gpimhip_ivr_greedy_banded on the handle H, as test_gpu_ivr_greedy.greedy_abi"""
    M = G.shape[0]
    m = spec.struct()
    Xd, yd, ud, Gd, wd, md = dev(X), dev(y), u.cuda(), dev(G), dev(w), dev(mask)
    f = lambda n: torch.full((n + 3,), -7.0, dtype=torch.float64, device="cuda")
    gain, maps, mean, sd, after = f(q), f(q * M), f(M), f(M), f(M)
    idx = torch.full((q + 3,), -7, dtype=torch.int64, device="cuda")
    count = torch.full((1 + 3,), -7, dtype=torch.int64, device="cuda")
    opt = lambda t: _lib.ptr(t) if want else None
    _lib.check(H.lib.gpimhip_ivr_greedy_banded(H.h, ctypes.byref(m), _lib.ptr(Xd), _lib.ptr(yd), X.shape[0], _lib.ptr(ud),
                                               _lib.ptr(Gd), M, band, _lib.ptr(wd), _lib.ptr(md), q, opt(mean), opt(sd),
                                               opt(maps), opt(after), _lib.ptr(idx), _lib.ptr(gain), _lib.ptr(count)))
    out = {}
    for name, t, n in (("idx", idx, q), ("gain", gain, q), ("count", count, 1), ("maps", maps, q * M), ("mean", mean, M),
                       ("sd", sd, M), ("sd_after", after, M)):
        h = t.cpu().numpy()
        assert np.all(h[n:] == -7), name
        out[name] = h[:n] if want or name in ("idx", "gain", "count") else None
    if want:
        out["maps"] = out["maps"].reshape(q, M)
    return out


def block_zero_weights(M):
    """weights with a whole block column of zeros and zeros across a block boundary"""
    w = np.linspace(0.5, 1.5, M)
    w[128:256] = 0.0
    w[380:390] = 0.0
    return w


# (kind, N, grid shape, bands, reference, weights): DESIGN.md section 30's table
EXACT = [("Matern52", 300, (25, 25), (1, 2, 3, 5, 7), "closed", None),      # five block columns, the last holding 113:
         #                                                                    2+2+1, 3+2, one band, clipped
         ("Matern52", 300, (25, 25), (2,), "closed", 7),                    # weights(M, 7)
         ("Matern52", 300, (25, 25), (2,), "closed", "zeros"),              # a block column of zero weights
         ("Matern52", 530, (20, 15), (1, 2), "closed", None),               # np = 640, 18-row ragged block; three block columns
         ("RBF", 40, (6, 5), (1,), "brute", None),                          # less than one tile
         ("Matern52", 40, (6, 5), (1,), "brute", None),
         ("RationalQuadratic", 40, (6, 5), (1,), "brute", None),
         ("RBF", 4, (25, 25), (2,), "closed", None),                        # the first step of a campaign
         ("Matern52", 130, (6, 5, 5), (1,), "brute", None)]                 # d = 3


@pytest.mark.parametrize("kind,N,shape,bands,how,wsel", EXACT,
                         ids=["%s-%d-%s-w%s" % (c[0], c[1], "x".join(map(str, c[2])), c[5]) for c in EXACT])
def test_exact_banded(eng, kind, N, shape, bands, how, wsel):
    _lib, H = eng
    kp, spec, u, X, y, G = IO.case(kind, N, shape)
    M = G.shape[0]
    assert len(X) == N
    if wsel == "zeros":
        w = block_zero_weights(M)
        ref = IO.closed(kp, X, G, w)
    else:
        w = None if wsel is None else IO.weights(M, wsel)
        ref = IO.reference(kind, N, shape, how, wsel)
    pm, pv = (t.numpy() for t in O.ExactGP(X, y, kp, IO.JITTER).predict(G))
    stored = ivr_abi(_lib, H, spec, u, X, y, G, w=w)
    first = None
    for band in bands:
        a, mean, sd = banded_abi(_lib, H, spec, u, X, y, G, band, w=w)
        check("%s N=%d grid %s weights %s band %d vs %s" % (kind, N, shape, wsel, band, how), a, ref)
        print("    max |mean - oracle| %.2e, max rel |sd^2 - oracle| %.2e; banded vs stored (acq, mean, sd): %s"
              % (np.abs(mean - pm).max(), np.abs(sd ** 2 / pv - 1).max(),
                 [np.abs(p - q).max() for p, q in zip((a, mean, sd), stored)]))
        assert np.abs(mean - pm).max() <= 1e-10 and np.abs(sd ** 2 / pv - 1).max() <= 1e-10
        assert all(np.array_equal(p, q) for p, q in zip((a, mean, sd), stored))
        first = first or (a, mean, sd)
        assert all(np.array_equal(p, q) for p, q in zip((a, mean, sd), first))      # every band width: the same bits
    # two identical calls: identical bits; outputs that are not wanted change nothing
    again = banded_abi(_lib, H, spec, u, X, y, G, bands[0], w=w)
    assert all(np.array_equal(p, q) for p, q in zip(again, first))
    assert np.array_equal(banded_abi(_lib, H, spec, u, X, y, G, bands[0], w=w, want_post=False)[0], first[0])


def test_mask_excludes_candidates_only(eng):
    _lib, H = eng
    kp, spec, u, X, y, G = IO.case("Matern52", 300, (25, 25))
    M = G.shape[0]
    mask = np.where(np.arange(M) % 7 == 3, np.nan, 1.0)
    a, mean, sd = banded_abi(_lib, H, spec, u, X, y, G, 2)
    am, mm, sm = banded_abi(_lib, H, spec, u, X, y, G, 2, mask=mask)
    keep = ~np.isnan(mask)
    assert np.isnan(am[~keep]).all() and np.array_equal(am[keep], a[keep]) and np.array_equal(mm, mean) and np.array_equal(sm, sd)


def fitted_600(_lib, used):
    """a handle that fitted N = 600: every row of the workspace written (DESIGN.md section 26's stale-W case)"""
    from gpim_amd.kernels import KernelSpec
    X6, y6 = IO.scattered(600, 2, seed=600, grid=64)
    s6 = KernelSpec("RBF", 2, [[1., 1.], [20., 20.]], jitter=1e-5)
    u6 = s6.draw_initial_u(generator=torch.Generator().manual_seed(6)).cuda()
    m6 = s6.struct()
    X6d, y6d = X6.cuda().contiguous(), y6.cuda().contiguous()
    _lib.check(used.lib.gpimhip_fit_exact(used.h, ctypes.byref(m6), _lib.ptr(X6d), _lib.ptr(y6d), len(X6), _lib.ptr(u6), 0.1, 3,
                                          None, None))
    return s6, u6.cpu(), X6, y6


def test_stale_state(eng):
    """W is grow-only and shared by the stored and the banded entries: the g rows of a longer batch, a downdated C and the
    rows of a larger N must not reach a later call.  Every call on the used handle returns a fresh handle's bits."""
    _lib, H = eng
    kp, spec, u, X, y, G = IO.case("Matern52", 300, (25, 25))
    args = (spec, u, X, y, G)
    fresh, used = _lib.Handle(), _lib.Handle()
    try:
        f3 = greedy_banded_abi(_lib, fresh, *args, 3, 2)
        fe = banded_abi(_lib, fresh, *args, 2)
        fs = ivr_abi(_lib, fresh, *args)
        fg = greedy_abi(_lib, fresh, *args, 3)
        greedy_banded_abi(_lib, used, *args, 8, 2)
        assert same_bits(greedy_banded_abi(_lib, used, *args, 3, 2), f3)            # q = 8, then q = 3
        greedy_banded_abi(_lib, used, *args, 8, 2)
        assert all(np.array_equal(p, q) for p, q in zip(banded_abi(_lib, used, *args, 2), fe))
        greedy_banded_abi(_lib, used, *args, 8, 2)
        assert all(np.array_equal(p, q) for p, q in zip(ivr_abi(_lib, used, *args), fs))
        greedy_banded_abi(_lib, used, *args, 8, 2)
        assert same_bits(greedy_abi(_lib, used, *args, 3), fg)
        # the stored greedy batch leaves a downdated C behind; the banded entries do not read it
        greedy_abi(_lib, used, *args, 8)
        assert all(np.array_equal(p, q) for p, q in zip(banded_abi(_lib, used, *args, 2), fe))
    finally:
        fresh.close()
        used.close()


def test_ragged_block_and_stale_padding(eng):
    """section 26's case through the banded entries: a handle that fitted N = 600 and ran banded calls of that order returns
    at N = 530 (np = 640, 18 valid rows in the last block) the bits of a fresh handle"""
    _lib, H = eng
    kp, spec, u, X, y, G = IO.case("Matern52", 530, (20, 15))
    fresh, used = _lib.Handle(), _lib.Handle()
    try:
        s6, u6, X6, y6 = fitted_600(_lib, used)
        banded_abi(_lib, used, s6, u6, X6, y6, G, 2)
        greedy_banded_abi(_lib, used, s6, u6, X6, y6, G, 6, 2)
        b = banded_abi(_lib, fresh, spec, u, X, y, G, 2)
        c = banded_abi(_lib, used, spec, u, X, y, G, 2)
        bg = greedy_banded_abi(_lib, fresh, spec, u, X, y, G, 6, 2)
        cg = greedy_banded_abi(_lib, used, spec, u, X, y, G, 6, 2)
    finally:
        fresh.close()
        used.close()
    assert all(np.array_equal(p, q) for p, q in zip(b, c)) and same_bits(bg, cg)
    check("Matern52 N=530 grid 20x15 band 2, used handle, vs closed", c[0], IO.reference("Matern52", 530, (20, 15), "closed"))


def test_memory_and_refusals(ensure_built):
    """The point of the feature: at M = 625 with band = 1 the handle holds C's four other block columns less.  A refused call
    allocates nothing."""
    from gpim_amd import _lib
    kp, spec, u, X, y, G = IO.case("Matern52", 300, (25, 25))
    M, m = G.shape[0], spec.struct()
    Hb, Hs, H32 = _lib.Handle(), _lib.Handle(), _lib.Handle(precision="single")
    try:
        banded_abi(_lib, Hb, spec, u, X, y, G, 1)
        ivr_abi(_lib, Hs, spec, u, X, y, G)
        bb, bs = Hb.lib.gpimhip_workspace_bytes(Hb.h), Hs.lib.gpimhip_workspace_bytes(Hs.h)
        print("workspace after the banded call (band = 1) %d bytes, after the stored call %d: %d fewer (C's other block "
              "columns: %d)" % (bb, bs, bs - bb, 8 * (640 - 128) * 640))
        assert bs - bb >= 8 * (640 - 128) * 640
        Xd, yd, ud, Gd = dev(X), dev(y), u.cuda(), dev(G)
        out = torch.zeros(M, dtype=torch.float64, device="cuda")
        idx, cnt = torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")

        def exact(handle=Hb, band=1, Xp=Xd, n=M):
            return handle.lib.gpimhip_ivr_exact_banded(handle.h, ctypes.byref(m), _lib.ptr(Xp), _lib.ptr(yd), X.shape[0],
                                                       _lib.ptr(ud), _lib.ptr(Gd), n, band, None, None, None, None,
                                                       _lib.ptr(out))

        def greedy(handle=Hb, band=1, Xp=Xd, q=2, idx_=idx):
            return handle.lib.gpimhip_ivr_greedy_banded(handle.h, ctypes.byref(m), _lib.ptr(Xp), _lib.ptr(yd), X.shape[0],
                                                        _lib.ptr(ud), _lib.ptr(Gd), M, band, None, None, q, None, None, None,
                                                        None, _lib.ptr(idx_), _lib.ptr(out), _lib.ptr(cnt))
        for fn, name in ((exact, "gpimhip_ivr_exact_banded"), (greedy, "gpimhip_ivr_greedy_banded")):
            cases = [(dict(band=0), "band = 0"), (dict(band=-1), "band = -1"), (dict(handle=H32), "double-precision"),
                     (dict(Xp=None), "null")]
            if fn is greedy:
                cases += [(dict(q=0), "q = 0"), (dict(q=M + 1), "q = %d" % (M + 1)), (dict(idx_=None), "idx_out")]
            else:
                cases += [(dict(n=2 ** 20 + 1), "M^2 / 128")]
            for kw, word in cases:
                h = kw.get("handle", Hb)
                b0 = h.lib.gpimhip_workspace_bytes(h.h)
                assert fn(**kw) == _lib.E_BADARG, (name, kw)
                err = h.lib.gpimhip_last_error().decode()
                assert err.startswith(name) and word in err, (kw, err)
                assert h.lib.gpimhip_workspace_bytes(h.h) == b0
        twoc = (ctypes.c_double * 4)(0, 0, 0, 0)
        assert Hb.lib.gpimhip_set_reflection(Hb.h, 1, twoc, None, X.shape[0], 0) == _lib.OK
        assert exact() == _lib.E_BADARG and "reflection" in Hb.lib.gpimhip_last_error().decode()
        assert Hb.lib.gpimhip_set_reflection(Hb.h, 0, twoc, None, 0, 0) == _lib.OK
        # a fresh handle refuses band = 0 without allocating anything
        Hn = _lib.Handle()
        try:
            n0 = Hn.lib.gpimhip_workspace_bytes(Hn.h)
            assert exact(handle=Hn, band=0) == _lib.E_BADARG and Hn.lib.gpimhip_workspace_bytes(Hn.h) == n0
        finally:
            Hn.close()
        # the band buffer and the g rows are counted and released with the rest
        assert greedy(q=3) == _lib.OK and cnt.item() == 3
        b1 = Hb.lib.gpimhip_workspace_bytes(Hb.h)
        assert Hb.lib.gpimhip_set_precision(Hb.h, 32) == 0
        assert Hb.lib.gpimhip_workspace_bytes(Hb.h) <= b1 - 8 * (640 * 144 + (384 + 128) * 656 + 5 * 640)
    finally:
        Hb.close()
        Hs.close()
        H32.close()


# (kind, N, grid shape, q, bands): section 30's greedy table
GREEDY = [("Matern52", 300, (25, 25), 8, (1, 2, 5)), ("Matern52", 530, (20, 15), 6, (2,)), ("RBF", 4, (25, 25), 32, (2,))]


@pytest.mark.parametrize("kind,N,shape,q,bands", GREEDY, ids=["%s-%d-q%d" % (c[0], c[1], c[3]) for c in GREEDY])
def test_greedy_banded(eng, kind, N, shape, q, bands):
    _lib, H = eng
    kp, spec, u, X, y, G = IO.case(kind, N, shape)
    M = G.shape[0]
    ref = GO.reference(kind, N, shape, q)
    assert len(ref.picks) == q
    after = GO.refit_variance(kp, X, G, ref.picks)
    stored = greedy_abi(_lib, H, spec, u, X, y, G, q)
    for band in bands:
        got = greedy_banded_abi(_lib, H, spec, u, X, y, G, q, band)
        check_against("%s N=%d grid %s q=%d band %d" % (kind, N, shape, q, band), got, ref, q, M, after_ref=after)
        assert got["count"][0] == q and np.array_equal(got["idx"], stored["idx"])
        print("    banded vs stored batch: maps %.2e of max a, sd_after %.2e"
              % (np.nanmax(np.abs(got["maps"] - stored["maps"])) / np.nanmax(ref.maps[0]),
                 np.abs(got["sd_after"] - stored["sd_after"]).max()))
        # round 0 is the exact entry, whichever: the same bits
        assert np.array_equal(got["maps"][0], stored["maps"][0]) and np.array_equal(got["mean"], stored["mean"])
        assert np.array_equal(got["sd"], stored["sd"]) and (got["sd_after"] <= got["sd"]).all()
        assert same_bits(got, greedy_banded_abi(_lib, H, spec, u, X, y, G, q, band))
    lean = greedy_banded_abi(_lib, H, spec, u, X, y, G, q, bands[0], want=False)
    assert np.array_equal(lean["idx"], ref.picks) and lean["maps"] is None


def test_greedy_one_pick_mask_and_ties(eng):
    _lib, H = eng
    kp, spec, u, X, y, G = IO.case("Matern52", 300, (25, 25))
    M = G.shape[0]
    # q = 1 returns gpimhip_ivr_exact_banded's bits, with weights and a mask
    for w, mask in ((None, None), (IO.weights(M, 7), np.where(np.arange(M) % 7 == 3, np.nan, 1.0))):
        a, mean, sd = banded_abi(_lib, H, spec, u, X, y, G, 2, w=w, mask=mask)
        got = greedy_banded_abi(_lib, H, spec, u, X, y, G, 1, 2, w=w, mask=mask)
        assert np.array_equal(got["maps"][0], a, equal_nan=True) and np.array_equal(got["mean"], mean)
        assert np.array_equal(got["sd"], sd) and got["count"][0] == 1 and got["gain"][0] == np.nanmax(a)
        rel = np.abs(got["sd_after"] ** 2 / GO.refit_variance(kp, X, G, got["idx"]) - 1.0).max()
        print("q = 1: pick %d, sd_after^2 against the refit's predict: max rel %.2e" % (got["idx"][0], rel))
        assert rel <= BAR
    # zero weights: every value ties at 0 in every round, the largest live flat index is taken
    tie = greedy_banded_abi(_lib, H, spec, u, X, y, G, 3, 2, w=np.zeros(M))
    assert tie["idx"].tolist() == [M - 1, M - 2, M - 3] and (tie["gain"] == 0.0).all() and tie["count"][0] == 3
    # the mask of tests/test_gpu_ivr_greedy.py that leaves three live candidates, six picks asked for
    kp, spec, u, X, y, G = IO.case("Matern52", 130, (13, 10))
    few = np.full(130, np.nan)
    few[[4, 77, 129]] = 1.0
    ref = GO.greedy(kp, X, G, 6, mask=few)
    got = greedy_banded_abi(_lib, H, spec, u, X, y, G, 6, 2, mask=few)
    check_against("3 live candidates, q = 6, band 2", got, ref, 6, 130, after_ref=GO.refit_variance(kp, X, G, ref.picks))
    assert got["count"][0] == 3 and sorted(got["idx"][:3].tolist()) == [4, 77, 129]
    assert np.all(got["idx"][3:] == -1) and np.isnan(got["gain"][3:]).all()


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


def test_reconstructor_band(fitted):
    gpim_amd, r, R = fitted
    Xf = gpim_amd.utils.get_full_grid(R)
    stored = r.ivr()
    for band in (1, 2, "auto", np.int64(1)):
        got = r.ivr(band=band)
        assert all(np.array_equal(p, q) for p, q in zip(got, stored)), band
    check("reconstructor.ivr(band=1) 16x16 vs closed", r.ivr(band=1)[0].ravel(), host_ivr(r, Xf))
    w = IO.weights(256, 3).reshape(16, 16)
    assert np.array_equal(r.ivr(weights=w, band=1)[0], r.ivr(weights=w)[0])
    points, gains, maps = r.ivr_batch(5, band=1)
    check_surface("ivr_batch(5, band=1) 16x16", points, gains, maps, host_greedy(r, Xf, 5), (16, 16))
    assert np.array_equal(maps["ivr"][0], stored[0]) and points == r.ivr_batch(5)[0]
    assert (maps["sd_after"] <= maps["sd"]).all() and np.isfinite(maps["sd_after"]).all()
    mask = np.ones((16, 16))
    mask[:, :3] = np.nan
    pw, gw, mw = r.ivr_batch(5, weights=w, mask=mask, band=2)
    check_surface("ivr_batch(5, band=2) 16x16, weights and mask", pw, gw, mw, host_greedy(r, Xf, 5, w, mask), (16, 16))
    acq, (mean, sd) = gpim_amd.acqfunc.integrated_variance_reduction(r, Xf, band=1)
    assert np.array_equal(acq, stored[0]) and np.array_equal(mean, stored[1]) and np.array_equal(sd, stored[2])
    for bad in (0, -1, 2.5, "x"):
        with pytest.raises(ValueError, match="band"):
            r.ivr(band=bad)
        with pytest.raises(ValueError, match="band"):
            r.ivr_batch(3, band=bad)
        with pytest.raises(ValueError, match="band"):
            gpim_amd.acqfunc.integrated_variance_reduction(r, Xf, band=bad)


def test_refusals_of_the_surface(fitted, tmp_path):
    gpim_amd, r, R = fitted
    Xs, Xf = gpim_amd.utils.get_sparse_grid(R), gpim_amd.utils.get_full_grid(R)
    _, full = image16()
    models = [(gpim_amd.reconstructor(Xs, R, Xf, precision="single", iterations=1, verbose=0), "single precision"),
              (gpim_amd.reconstructor(Xs, R, Xf, sparse=True, indpoints=20, iterations=1, verbose=0), "inducing points"),
              (gpim_amd.reconstructor(Xf, full, Xf, structured=True, iterations=1, verbose=0), "not block-structured")]
    for model, why in models:
        with pytest.raises(NotImplementedError, match=why):
            model.ivr(band=1)
        with pytest.raises(NotImplementedError, match=why):
            model.ivr_batch(3, band=1)
    kw = dict(acquisition_function="ivr", exploration_steps=1, gp_iterations=1, verbose=0, filename=str(tmp_path / "bo"))
    for bad in (0, -1, 2.5, "x"):
        with pytest.raises(ValueError, match="band"):
            gpim_amd.boptimizer(Xs, R.copy(), Xf, lambda idx: 0.0, ivr_band=bad, **kw)
    with pytest.raises(NotImplementedError):
        gpim_amd.boptimizer(Xs, R.copy(), Xf, lambda idx: 0.0, ivr_band=1, precision="single", **kw)
    # the option belongs to 'ivr' alone, as ivr_batch
    gpim_amd.boptimizer(Xs, R.copy(), Xf, lambda idx: 0.0, **dict(kw, acquisition_function="cb", ivr_band="x"))
    gpim_amd.boptimizer(Xs, R.copy(), Xf, lambda idx: 0.0, ivr_band="auto", **kw)


def test_boptimizer_band(ensure_built, tmp_path):
    """boptimizer('ivr', ivr_band=1) on C4's 25 x 25 problem: every pick has the host closed form's maximum"""
    import gpim_amd
    bo, maps = campaign(gpim_amd, tmp_path, "ivr", ivr_band=1)
    bo.run()
    assert len(bo.indices_all) == 3 and len(maps) == 3
    check_picks("'ivr', ivr_band=1", bo, maps, bo.indices_all)
    for mean, sd in bo.gp_predictions:
        assert mean.shape == sd.shape == (25, 25) and np.isfinite(mean).all() and (sd > 0).all()


def test_boptimizer_greedy_band(ensure_built, tmp_path):
    """batch_update=True, ivr_batch='greedy', ivr_band=2, batch_out_max=4: every step's batch is the host greedy batch at
    that step's hyper-parameters"""
    import gpim_amd
    bo, refs = greedy_campaign(gpim_amd, tmp_path, ivr_batch="greedy", ivr_band=2, batch_out_max=4)
    bo.run()
    assert len(refs) == 3 and len(bo.indices_all) == 12 and len(bo.vals_all) == 12
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


def test_boptimizer_default_is_the_stored_path(ensure_built, tmp_path):
    """ivr_band=None and no option at all return the ranked map of ivr_on_device without a band, value for value"""
    import gpim_amd
    from gpim_amd import acqfunc
    out = []
    for kw in ({}, dict(ivr_band=None)):
        bo, _ = campaign(gpim_amd, tmp_path, "ivr", **kw)
        assert bo.ivr_band is None
        bo.surrogate_model.train()
        vals, inds = bo.__class__.next_point(bo)
        acq_d, _, _ = acqfunc.ivr_on_device(bo.surrogate_model, bo._Xfull_d)
        rv, ri = bo._rank_device(acq_d, (25, 25), masked=True)
        assert vals == rv and inds == ri
        out.append((vals, inds))
    assert out[0] == out[1]
