"""
The banded integrated variance reduction without a GPU (gpimhip_ivr_exact_banded, gpimhip_ivr_greedy_banded; DESIGN.md
section 30):

(a) acqfunc._ivr_band, the one host function that resolves the `band` argument of the Python surface;
(b) the two entries are exported by the built library with the arguments of their declarations in include/gpimhip.h;
(c) the mathematics of the banded greedy batch, in numpy, on every case of tests/ivr_greedy_oracle.py: without a stored C a
    pick is conditioned on by appending g = c / sqrt(max(c_p, 0) + noise + jitter), c = k(G, g_p) - W_aug^T W_aug[:, p], to
    W as one more row, and the map of round r is tests/ivr_oracle.py's `closed` formula on K(G, G) - W_aug^T W_aug.  These
    maps must equal the maps of `greedy` (C downdated in place) round by round.  Bar: 1e-12 of the round-0 maximum, the bar
    tests/test_ivr_greedy_host.py holds `greedy` to the refits with (it measures <= 7.6e-15 there); measured here
    <= 1.3e-14 (Matern52, N = 530), the picks equal in every round.

Every test prints what it measured before it asserts.
"""
import os
import re

import numpy as np
import pytest
import torch

import ivr_oracle as IO
import ivr_greedy_oracle as GO
from test_ivr_greedy_host import ident

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ivr_band():
    from gpim_amd.acqfunc import _ivr_band
    assert _ivr_band(None, 625) is None
    assert _ivr_band(3, 625) == 3 and _ivr_band(np.int64(3), 625) == 3
    assert _ivr_band("auto", 16384) is None
    assert _ivr_band("auto", 16385) == 2 ** 28 // (128 * 16512)         # the first size past the stored limit
    assert _ivr_band("auto", 65536) == 32
    assert _ivr_band("auto", 262144) == 8
    assert _ivr_band("auto", 2 ** 22) == 1                              # never less than one block column
    for bad in (0, -1, 2.5, "x", True):
        with pytest.raises(ValueError, match="band"):
            _ivr_band(bad, 625)


@pytest.mark.parametrize("name,after_m,n", [("gpimhip_ivr_exact_banded", "gpimhip_ivr_exact", 14),
                                            ("gpimhip_ivr_greedy_banded", "gpimhip_ivr_greedy", 19)])
def test_entries_are_exported(name, after_m, n):
    """exported with the arguments of the stored entry plus `band` behind M, as include/gpimhip.h declares them"""
    from gpim_amd import _lib
    assert name in _lib.EXPORTS
    with open(os.path.join(ROOT, "include", "gpimhip.h")) as f:
        text = f.read()
    args = lambda fn: [a.split()[-1].lstrip("*") for a in re.search(r"int %s\(([^;]*)\);" % fn, text).group(1).split(",")]
    names, stored = args(name), args(after_m)
    at = stored.index("M") + 1
    assert names == stored[:at] + ["band"] + stored[at:]
    assert len(_lib._PROTOS[name][1]) == len(names) == n


def augmented_maps(kp, X, G, picks, w=None, jitter=IO.JITTER):
    """(maps (q, M), picks the maps lead to, diag of the last C): the banded batch in numpy, conditioning on picks[r]"""
    with torch.no_grad():
        K = kp.K(X).numpy().copy()
        Ks = kp.K(X, G).numpy()
        Kss = kp.K(G).numpy()
        noise = kp.noise.item()
    K[np.diag_indices(K.shape[0])] += jitter + noise
    Wa = np.linalg.solve(np.linalg.cholesky(K), Ks)
    M = Kss.shape[0]
    w = np.ones(M) if w is None else np.asarray(w, dtype=np.float64)
    live = np.ones(M)
    maps, own = [], []
    for p in picks:
        C = Kss - Wa.T @ Wa
        C = 0.5 * (C + C.T)
        a = live * ((w[:, None] * C * C).sum(0) / (np.maximum(np.diag(C), 0.0) + noise + jitter))
        maps.append(a)
        ok = np.flatnonzero(~np.isnan(a))
        own.append(int(ok[a[ok] == a[ok].max()].max()))
        live[p] = np.nan
        c = Kss[:, p] - Wa.T @ Wa[:, p]
        Wa = np.vstack([Wa, c / np.sqrt(max(c[p], 0.0) + noise + jitter)])
    return np.array(maps), own, np.diag(Kss - Wa.T @ Wa)


@pytest.mark.parametrize("kind,N,shape,q,wseed", GO.CASES, ids=[ident(c) for c in GO.CASES])
def test_augmented_w_is_the_downdate(kind, N, shape, q, wseed):
    kp, _, _, X, _, G = IO.case(kind, N, shape)
    w = None if wseed is None else IO.weights(G.shape[0], wseed)
    ref = GO.reference(kind, N, shape, q, wseed)
    maps, own, diag = augmented_maps(kp, X, G, ref.picks, w)
    on = ~np.isnan(ref.maps)
    top = np.nanmax(ref.maps[0])
    gap = np.abs(maps - ref.maps)[on].max()
    dgap = np.abs(diag - ref.diag).max()
    print("%s N=%d grid %s q=%d weights %s: max a %.4f, max |K - Waug^T Waug maps - downdated maps| %.2e = %.2e of max a; "
          "final diagonal %.2e" % (kind, N, shape, q, wseed, top, gap, gap / top, dgap))
    assert np.array_equal(np.isnan(maps), ~on)
    assert own == ref.picks.tolist()
    assert gap <= 1e-12 * top
    assert dgap <= 1e-12 * ref.diag.max()
