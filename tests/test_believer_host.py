"""
Believer batches of CB / EI / POI without a GPU (tests/believer_oracle.py), on every case and setting the GPU tests run:

(a) the maps of the scheme (conditioned columns from W alone) equal the maps of the refitted model (the definition, the
    incumbents of EI / POI included) to 1e-12 of the largest |value| of the round-0 map, at the live entries -- the
    identity is exact, the bar is that of tests/test_ivr_greedy_host.py; measured <= 4.6e-14;
(b) the condition of the GPU tests' pick comparison: in every round the best live value leads the second best by >= 1e-7
    relative, a thousand times the 1e-10 bar the GPU maps are held to (smallest gap measured: 1.9e-7, RBF, N = 4, grid
    25 x 25, q = 32, CB(0, 1));
(c) the latent variance stays > 0 through all rounds, so the clamp at 0 cannot hide a difference (smallest: 5.5e-3);
(d) the final variance is the refit's;
(e) the library's export table.

Every test prints what it measured before it asserts.
"""
import os
import re

import numpy as np
import pytest

import ivr_oracle as IO
import believer_oracle as BO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = [(c, s) for c in BO.CASES for s in BO.SETTINGS]


@pytest.mark.parametrize("case,setting", GRID, ids=[BO.ident(c, s) for c, s in GRID])
def test_scheme_is_the_refit_and_picks_are_clear(case, setting):
    kind, N, shape, q = case
    kp, _, _, X, y, G = IO.case(kind, N, shape)
    assert len(X) == N
    M = G.shape[0]
    ref = BO.reference(*case, *setting)
    assert len(ref.picks) == q and len(set(ref.picks.tolist())) == q and ref.maps.shape == (q, M)
    refit = BO.refit_maps(kp, X, y, G, ref.picks, *setting)
    on = ~np.isnan(ref.maps)
    top = np.nanmax(np.abs(ref.maps[0]))
    gap = np.abs(ref.maps - refit)[on].max()
    print("%s: max |map 0| %.4g, max |scheme - refit| %.2e = %.2e of it; smallest gap %.2e, smallest v %.3e"
          % (BO.ident(case, setting), top, gap, gap / top, ref.gaps.min(), ref.v_min))
    for r in range(q):
        assert np.array_equal(np.flatnonzero(~on[r]), np.sort(ref.picks[:r]))           # NaN exactly at the earlier picks
    assert np.array_equal(np.isnan(refit), ~on)
    assert gap <= 1e-12 * top
    assert ref.gaps.min() >= 1e-7
    assert ref.v_min > 0.0
    after = BO.refit_variance(kp, X, G, ref.picks)
    assert np.abs(ref.v + ref.noise - after).max() <= 1e-10 * after.max()


def test_mask_and_exhaustion():
    """masked candidates are never picked; with 3 live candidates and q = 6 the scheme stops after 3"""
    case = ("Matern52", 130, (13, 10), 8)
    kp, _, _, X, y, G = IO.case(*case[:3])
    M = G.shape[0]
    for setting in BO.SETTINGS:
        free = BO.reference(*case, *setting)
        mask = np.ones(M)
        mask[free.picks[:3]] = np.nan
        ref = BO.scheme(kp, X, y, G, 8, *setting, mask=mask)
        assert len(ref.picks) == 8 and not set(ref.picks.tolist()) & set(free.picks[:3].tolist())
        assert np.isnan(ref.maps[:, free.picks[:3]]).all()
        refit = BO.refit_maps(kp, X, y, G, ref.picks, *setting, mask=mask)
        on = ~np.isnan(ref.maps)
        assert np.abs(ref.maps - refit)[on].max() <= 1e-12 * np.nanmax(np.abs(ref.maps[0]))
        few = np.full(M, np.nan)
        few[[4, 77, 129]] = 1.0
        ref = BO.scheme(kp, X, y, G, 6, *setting, mask=few)
        assert sorted(ref.picks.tolist()) == [4, 77, 129] and len(ref.vals) == 3 and ref.maps.shape == (3, M)


def test_entry_is_exported():
    """gpimhip_acquire_batch is exported with the 22 arguments of its declaration in include/gpimhip.h"""
    from gpim_amd import _lib
    assert "gpimhip_acquire_batch" in _lib.EXPORTS
    with open(os.path.join(ROOT, "include", "gpimhip.h")) as f:
        decl = re.search(r"int gpimhip_acquire_batch\(([^;]*)\);", f.read()).group(1)
    names = [a.split()[-1].lstrip("*") for a in decl.split(",")]
    assert names == ["h", "m", "X", "y", "N", "u", "Xs", "M", "Xobs", "Mobs", "kind", "p0", "p1", "mask", "q", "mean_out",
                     "sd_out", "maps_out", "sd_after_out", "idx_out", "val_out", "count_out"]
    assert len(_lib._PROTOS["gpimhip_acquire_batch"][1]) == len(names) == 22
