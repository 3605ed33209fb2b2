"""
The greedy batch of integrated variance reduction without a GPU (tests/ivr_greedy_oracle.py), on every case the GPU tests run:

(a) the maps of the downdated covariance equal the maps of the refitted model (the definition) to 1e-12 of the round-0 maximum
    -- the identity is exact, the bar is that of tests/test_ivr_host.py; measured <= 7.6e-15;
(b) the condition of the GPU tests' pick comparison: in every round the best live value leads the second best by >= 1e-6
    relative, four orders above the 1e-10 bar the GPU maps are held to, so an engine inside its bar cannot flip a pick
    (smallest gap measured: 8.4e-5); and diag(C) stays > 0 through all rounds (>= 1.3e-2), so the clamp at 0 cannot hide a
    difference;
(c) the gains of a batch add up to its total drop: sum_r gain_r = sum_m w_m (var_before(m) - var_after(m)) from two
    predictions of the dense oracle, the second with the whole batch appended.  Bar: 1e-10 of sum_m w_m var_before(m), the
    project's relative bar for a dense double variance applied to what is subtracted;
(d) the library's export table.

Every test prints what it measured before it asserts.
"""
import os
import re

import numpy as np
import pytest
import torch

from oracle import gpim_oracle as O
import ivr_oracle as IO
import ivr_greedy_oracle as GO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ident(c):
    return "%s-%d-%s-q%d-w%s" % (c[0], c[1], "x".join(map(str, c[2])), c[3], c[4])


@pytest.mark.parametrize("kind,N,shape,q,wseed", GO.CASES, ids=[ident(c) for c in GO.CASES])
def test_downdate_is_the_refit_and_picks_are_clear(kind, N, shape, q, wseed):
    kp, _, _, X, _, G = IO.case(kind, N, shape)
    assert len(X) == N
    M = G.shape[0]
    w = None if wseed is None else IO.weights(M, wseed)
    ref = GO.reference(kind, N, shape, q, wseed)
    assert len(ref.picks) == q and len(set(ref.picks.tolist())) == q and ref.maps.shape == (q, M)
    # (a)
    refit = GO.refit_maps(kp, X, G, ref.picks, w)
    on = ~np.isnan(ref.maps)
    top = np.nanmax(ref.maps[0])
    gap = np.abs(ref.maps - refit)[on].max()
    # (b)
    print("%s N=%d grid %s q=%d weights %s: max a %.4f, max |downdate - refit| %.2e = %.2e of max a; smallest gap %.2e, "
          "smallest diag(C) %.3e" % (kind, N, shape, q, wseed, top, gap, gap / top, ref.gaps.min(), ref.diag_min))
    for r in range(q):
        assert np.array_equal(np.flatnonzero(~on[r]), np.sort(ref.picks[:r]))           # NaN exactly at the earlier picks
    assert gap <= 1e-12 * top
    assert ref.gaps.min() >= 1e-6
    assert ref.diag_min > 0.0
    # (c)
    wv = np.ones(M) if w is None else w
    before = O.ExactGP(X, torch.zeros(N, dtype=torch.float64), kp, IO.JITTER).predict(G)[1].numpy()
    after = GO.refit_variance(kp, X, G, ref.picks)
    drop, scale = np.sum(wv * (before - after)), np.sum(wv * before)
    print("    sum of gains %.12g, drop of the weighted total variance %.12g, difference %.2e = %.2e of sum w var_before"
          % (ref.gains.sum(), drop, abs(ref.gains.sum() - drop), abs(ref.gains.sum() - drop) / scale))
    assert abs(ref.gains.sum() - drop) <= 1e-10 * scale
    # the final diagonal is the refit's latent variance
    assert np.abs(ref.diag + ref.noise - after).max() <= 1e-10 * after.max()


def test_mask_and_exhaustion():
    """masked candidates are never picked; with 3 live candidates and q = 6 the oracle stops after 3"""
    kind, N, shape = "Matern52", 130, (13, 10)
    kp, _, _, X, _, G = IO.case(kind, N, shape)
    M = G.shape[0]
    free = GO.reference(kind, N, shape, 8)
    mask = np.ones(M)
    mask[free.picks[:3]] = np.nan
    ref = GO.greedy(kp, X, G, 8, mask=mask)
    assert len(ref.picks) == 8 and not set(ref.picks.tolist()) & set(free.picks[:3].tolist())
    assert np.isnan(ref.maps[:, free.picks[:3]]).all()
    few = np.full(M, np.nan)
    few[[4, 77, 129]] = 1.0
    ref = GO.greedy(kp, X, G, 6, mask=few)
    assert sorted(ref.picks.tolist()) == [4, 77, 129] and len(ref.gains) == 3 and ref.maps.shape == (3, M)


def test_ties_go_to_the_larger_index():
    """weights of zero make every value 0: all candidates tie in every round and the largest live flat index is taken, as
    gpimhip_topk ranks"""
    kp, _, _, X, _, G = IO.case("Matern52", 130, (13, 10))
    with np.errstate(invalid="ignore"):
        ref = GO.greedy(kp, X, G, 3, w=np.zeros(130))
    assert ref.picks.tolist() == [129, 128, 127] and (ref.gains == 0.0).all()


def test_entry_is_exported():
    """gpimhip_ivr_greedy is exported with the 18 arguments of its declaration in include/gpimhip.h"""
    from gpim_amd import _lib
    assert "gpimhip_ivr_greedy" in _lib.EXPORTS
    with open(os.path.join(ROOT, "include", "gpimhip.h")) as f:
        decl = re.search(r"int gpimhip_ivr_greedy\(([^;]*)\);", f.read()).group(1)
    names = [a.split()[-1].lstrip("*") for a in decl.split(",")]
    assert names == ["h", "m", "X", "y", "N", "u", "Xs", "M", "weights", "mask", "q", "mean_out", "sd_out", "maps_out",
                     "sd_after_out", "idx_out", "gain_out", "count_out"]
    assert len(_lib._PROTOS["gpimhip_ivr_greedy"][1]) == len(names) == 18
