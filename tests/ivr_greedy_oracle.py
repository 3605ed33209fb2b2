"""
CPU references for the greedy batch of integrated variance reduction (reconstructor.ivr_batch, gpimhip_ivr_greedy), float64
throughout.  A GP's variance does not depend on the measured values: after picking p the latent covariance of the grid is
C - c c^T / (C_pp + noise + jitter), c = C[:, p], and the next map is tests/ivr_oracle.py's `closed` formula on the new C.

  greedy(kp, X, G, q, w, mask)        the engine's scheme in numpy: posterior_cov, then map / arg-max (NaN never, ties to the
                                      larger flat index) / C -= g g^T with g = c / sqrt(max(C_pp, 0) + noise + jitter)
  refit_maps(kp, X, G, picks, w)      the definition: closed(kp, X u G[picks[:r]], G, w) for every round r
  refit_variance(kp, X, G, picks)     predict's variance (noise included) of the dense oracle with the whole batch appended

The problems and grids are those of tests/ivr_oracle.py (imported, not copied).  tests/test_ivr_greedy_host.py holds greedy to
the refits without a GPU and shows that no pick of a case is closer to a tie than the GPU bar could flip; the GPU tests then
compare with greedy.
"""
import collections
import functools

import numpy as np
import torch

from oracle import gpim_oracle as O
import ivr_oracle as IO
from ivr_oracle import JITTER

Greedy = collections.namedtuple("Greedy", "picks gains maps diag gaps diag_min noise")

# (kind, N, grid shape, q, weights seed): the cases of tests/test_gpu_ivr_greedy.py and what each reaches
CASES = [("RBF", 40, (6, 5), 6, None),                  # less than one tile: the diagonal tile's mirrored downdate
         ("Matern52", 40, (6, 5), 6, None),
         ("RationalQuadratic", 40, (6, 5), 6, None),
         ("Matern52", 130, (13, 10), 8, None),          # two tiles, the second holding 2 columns: off-diagonal tile, row walk
         ("Matern52", 130, (13, 10), 8, 7),             # ... with zero weights
         ("Matern52", 130, (6, 5, 5), 8, None),         # d = 3
         ("Matern52", 300, (25, 25), 8, None),          # five tiles, the last holding 113 columns
         ("Matern52", 530, (20, 15), 6, None),          # ragged last block of W under a downdated C
         ("RBF", 4, (25, 25), 32, None)]                # many rounds: error growth, every tile rewritten 31 times


def greedy(kp, X, G, q, w=None, mask=None, jitter=JITTER):
    """Greedy(picks, gains, maps (q, M), diag: diag(C) after all picks, gaps: per round (best - second best live value) /
    best (inf with one live candidate), diag_min: the smallest diagonal entry seen in any round, noise).  mask: None or M
    values of 1 / NaN.  Stops early when no live candidate is left: the arrays then hold the rounds made."""
    C, noise = IO.posterior_cov(kp, X, G, jitter)
    M = C.shape[0]
    w = np.ones(M) if w is None else np.asarray(w, dtype=np.float64)
    live = np.ones(M) if mask is None else np.asarray(mask, dtype=np.float64).copy()
    picks, gains, maps, gaps, dmin = [], [], [], [], np.inf
    for _ in range(q):
        d = np.diag(C)
        dmin = min(dmin, d.min())
        a = live * ((w[:, None] * C * C).sum(0) / (np.maximum(d, 0.0) + noise + jitter))
        ok = np.flatnonzero(~np.isnan(a))
        if ok.size == 0:
            break
        best = a[ok].max()
        p = int(ok[a[ok] == best].max())
        rest = a[ok[ok != p]]
        gaps.append((best - rest.max()) / best if rest.size else np.inf)
        picks.append(p)
        gains.append(best)
        maps.append(a)
        live[p] = np.nan
        g = C[:, p] / np.sqrt(max(C[p, p], 0.0) + noise + jitter)
        C = C - np.outer(g, g)
    dmin = min(dmin, np.diag(C).min())
    return Greedy(np.array(picks, dtype=np.int64), np.array(gains), np.array(maps).reshape(len(maps), M), np.diag(C).copy(),
                  np.array(gaps), dmin, noise)


def refit_maps(kp, X, G, picks, w=None, jitter=JITTER):
    """(len(picks), M): row r = the closed-form map of the model refitted to X and the picks before round r"""
    return np.array([IO.closed(kp, torch.cat([X, G[np.array(picks[:r], dtype=np.int64)]]), G, w, jitter)
                     for r in range(len(picks))])


def refit_variance(kp, X, G, picks, jitter=JITTER):
    """predict's variance on G (noise included) with G[picks] appended to the training rows (y does not enter: zeros)"""
    Xa = torch.cat([X, G[np.array(picks, dtype=np.int64)]])
    return O.ExactGP(Xa, torch.zeros(Xa.shape[0], dtype=torch.float64), kp, jitter).predict(G)[1].numpy()


@functools.lru_cache(maxsize=None)
def reference(kind, N, shape, q, wseed=None):
    """greedy() of a case, computed once and shared (read-only arrays)"""
    kp, _, _, X, _, G = IO.case(kind, N, shape)
    w = None if wseed is None else IO.weights(G.shape[0], wseed)
    ref = greedy(kp, X, G, q, w)
    for a in ref[:5]:
        a.setflags(write=False)
    return ref
