"""
CPU references for believer batches of CB / EI / POI (reconstructor.acq_batch, gpimhip_acquire_batch), float64 throughout.
After picking p the model is conditioned on p having been measured at its posterior mean (kriging believer; GP-BUCB for
CB): the mean map does not change, the latent variance drops by tests/ivr_greedy_oracle.py's identity, and the next pick
maximises the acquisition function of the conditioned model.

  scheme(kp, X, y, G, q, kind, p0, p1, xi, mask)   the engine's four steps in numpy, from W = L^-1 K(X, G) alone: map / arg-max
                                                   (NaN never, ties to the larger flat index) / conditioned column
                                                   c = k(G, g_p) - W^T W[:, p] - sum_s g^(s) g^(s)[p], g = c / sqrt(max(c_p, 0)
                                                   + noise + jitter), v -= g o g / incumbent
  refit_maps(...)                                  the definition: for every round the dense oracle fitted to X u G[picks
                                                   before] with y u their posterior means, the reference's acquisition
                                                   formulas, the incumbent from `predict` at that model's own training rows
  refit_variance(kp, X, G, picks)                  tests/ivr_greedy_oracle.py's (imported)

The problems and grids are those of tests/ivr_oracle.py; the cases are the (kind, N, grid, q) of tests/ivr_greedy_oracle.py
(its weights do not enter, the duplicate drops), each with the four SETTINGS.  tests/test_believer_host.py holds scheme to
the refits without a GPU and shows that no pick is closer to a tie than the GPU bar could flip; the GPU tests compare with
scheme.
"""
import collections
import functools

import numpy as np
import torch
from scipy.stats import norm

from oracle import gpim_oracle as O
import ivr_oracle as IO
import ivr_greedy_oracle as GO
from ivr_oracle import JITTER
from ivr_greedy_oracle import refit_variance  # noqa: F401  (re-exported for the tests)

Believer = collections.namedtuple("Believer", "picks vals maps v gaps v_min noise mean sd")

# (kind, N, grid shape, q): what each reaches is listed in tests/test_gpu_believer.py
CASES = list(dict.fromkeys(c[:4] for c in GO.CASES))
# (acquisition, p0, p1, xi): CB reads (p0, p1) = (alpha, beta), EI / POI read xi
SETTINGS = [("cb", 0.0, 1.0, 0.01), ("cb", 1.0, 2.0, 0.01), ("ei", 0.0, 0.0, 0.01), ("poi", 0.0, 0.0, 0.01)]


def ident(c, s):
    return "%s-%d-%s-q%d-%s-%g-%g" % (c[0], c[1], "x".join(map(str, c[2])), c[3], s[0], s[1], s[2])


def acq(kind, mean, sd, p0, p1, xi, best):
    """the reference's formulas (gpim/gpbayes/acqfunc.py; oracle.gpim_oracle restates them around a model)"""
    if kind == "cb":
        return p0 * mean + p1 * sd
    imp = mean - best - xi
    z = imp / sd
    return imp * norm.cdf(z) + sd * norm.pdf(z) if kind == "ei" else norm.cdf(z)


def incumbent(kind, mean_obs, sd_obs):
    """nanmax of the posterior at the observed rows: means for EI, means and sds for POI (the reference's tuple quirk)"""
    if kind == "cb":
        return np.nan
    return np.nanmax(mean_obs) if kind == "ei" else np.nanmax(np.concatenate([mean_obs, sd_obs]))


def scheme(kp, X, y, G, q, kind, p0=0.0, p1=1.0, xi=0.01, mask=None, jitter=JITTER):
    """Believer(picks, vals, maps (rounds, M), v: the latent variance after all picks, gaps: per round (best - second best
    live value) / |best| (inf with one live candidate), v_min: the smallest latent variance seen, noise, mean, sd: the
    posterior before the batch).  Stops early when no live candidate is left: the arrays then hold the rounds made."""
    with torch.no_grad():
        K = kp.K(X).numpy().copy()
        Ks = kp.K(X, G).numpy()
        s2, noise = kp.variance.item(), kp.noise.item()
    N, M = Ks.shape
    K[np.diag_indices(N)] += jitter + noise
    L = np.linalg.cholesky(K)
    W = np.linalg.solve(L, Ks)
    alpha = np.linalg.solve(L.T, np.linalg.solve(L, y.numpy()))
    mean = Ks.T @ alpha
    v = s2 - (W * W).sum(0)
    sd0 = np.sqrt(np.maximum(v, 0.0) + noise)
    b = np.nan
    if kind != "cb":
        Wo = np.linalg.solve(L, K - (jitter + noise) * np.eye(N))
        sdo = np.sqrt(np.maximum(s2 - (Wo * Wo).sum(0), 0.0) + noise)
        b = incumbent(kind, (K - (jitter + noise) * np.eye(N)) @ alpha, sdo)
    live = np.ones(M) if mask is None else np.asarray(mask, dtype=np.float64).copy()
    picks, vals, maps, gaps, gs, vmin = [], [], [], [], [], v.min()
    for _ in range(q):
        a = live * acq(kind, mean, np.sqrt(np.maximum(v, 0.0) + noise), p0, p1, xi, b)
        ok = np.flatnonzero(~np.isnan(a))
        if ok.size == 0:
            break
        best = a[ok].max()
        p = int(ok[a[ok] == best].max())
        rest = a[ok[ok != p]]
        gaps.append((best - rest.max()) / abs(best) if rest.size else np.inf)
        picks.append(p)
        vals.append(best)
        maps.append(a)
        live[p] = np.nan
        with torch.no_grad():
            c = kp.K(G, G[p:p + 1]).numpy()[:, 0] - W.T @ W[:, p]
        for g in gs:
            c = c - g * g[p]
        g = c / np.sqrt(max(c[p], 0.0) + noise + jitter)
        gs.append(g)
        v = v - g * g
        vmin = min(vmin, v.min())
        if kind == "ei":
            b = np.fmax(b, mean[p])
        elif kind == "poi":
            b = np.fmax(np.fmax(b, mean[p]), np.sqrt(max(v[p], 0.0) + noise))
    return Believer(np.array(picks, dtype=np.int64), np.array(vals), np.array(maps).reshape(len(maps), M), v, np.array(gaps),
                    vmin, noise, mean, sd0)


def refit_maps(kp, X, y, G, picks, kind, p0=0.0, p1=1.0, xi=0.01, mask=None, jitter=JITTER):
    """(len(picks), M): row r = the acquisition map of the dense oracle refitted to X and the picks before round r, each
    pick with the posterior mean it had when it was made as its value; NaN at masked candidates and earlier picks"""
    M = G.shape[0]
    live = np.ones(M) if mask is None else np.asarray(mask, dtype=np.float64).copy()
    Xa, ya, rows = X, y, []
    for p in picks:
        gp = O.ExactGP(Xa, ya, kp, jitter)
        mean, var = (t.numpy() for t in gp.predict(G))
        mo, vo = (t.numpy() for t in gp.predict(Xa))
        rows.append(live * acq(kind, mean, np.sqrt(var), p0, p1, xi, incumbent(kind, mo, np.sqrt(vo))))
        live[p] = np.nan
        Xa = torch.cat([Xa, G[p:p + 1]])
        ya = torch.cat([ya, torch.from_numpy(mean[p:p + 1])])
    return np.array(rows).reshape(len(rows), M)


@functools.lru_cache(maxsize=None)
def reference(kind, N, shape, q, acqf, p0, p1, xi):
    """scheme() of a case and a setting, computed once and shared (read-only arrays)"""
    kp, _, _, X, y, G = IO.case(kind, N, shape)
    ref = scheme(kp, X, y, G, q, acqf, p0, p1, xi)
    for a in ref:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref
