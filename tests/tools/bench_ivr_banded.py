"""Times gpimhip_ivr_exact_banded next to gpimhip_ivr_exact, and the q = 10 greedy batches of both kinds, on bench_ivr.py's
problems: a warm handle, a host clock around a call that ends in a synchronise, the median of 10
calls with the variants alternated inside every repetition, (N, M) = (1024, 4096) and (4212, 16384); one JSON line per
case with the handle's workspace bytes after the banded calls alone (a second handle) and after all of them.
`--big`: (4212, 65536) -- C would be 34 GB -- with the banded call at 'auto''s band alone.
`--profile N M`: a few stored and banded calls at (N, M) only, for a run under `rocprofv3 --kernel-trace --stats`."""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
import torch

from gpim_amd import _lib
from gpim_amd.acqfunc import _ivr_band
from bench_ivr import problem


def timed(fns, reps):
    """{name: (median ms, min ms)}: two warm-up calls each, then `reps` repetitions that call every variant once, in order"""
    for fn in fns.values():
        fn()
        fn()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()                                    # (the entry synchronises its stream before it returns)
            ts[k].append(time.perf_counter() - t0)
    return {k: (1e3 * statistics.median(v), 1e3 * min(v)) for k, v in ts.items()}


def run(N, M, bands, reps=10, q=10, stored=True):
    spec, u, X, y, G = problem(N, M)
    m = spec.struct()
    nt = (M + 127) // 128
    H, Hb = _lib.Handle(), _lib.Handle()
    mean, sd, acq, after = (torch.empty(M, dtype=torch.float64, device="cuda") for _ in range(4))
    idx, cnt = torch.empty(q, dtype=torch.int64, device="cuda"), torch.empty(1, dtype=torch.int64, device="cuda")
    gain = torch.empty(q, dtype=torch.float64, device="cuda")
    head = lambda h: (h.h, ctypes.byref(m), _lib.ptr(X), _lib.ptr(y), N, _lib.ptr(u), _lib.ptr(G), M)
    out = (None, None, _lib.ptr(mean), _lib.ptr(sd), _lib.ptr(acq))
    gout = (None, None, q, _lib.ptr(mean), _lib.ptr(sd), None, _lib.ptr(after), _lib.ptr(idx), _lib.ptr(gain), _lib.ptr(cnt))
    res = {"N": N, "M": M, "q": q}
    # the banded calls alone on a handle of their own: what the feature needs
    _lib.check(Hb.lib.gpimhip_ivr_exact_banded(*head(Hb), min(bands), *out))
    res["workspace_bytes_banded_band%d" % min(bands)] = int(Hb.lib.gpimhip_workspace_bytes(Hb.h))
    res["acq_max_banded"] = float(acq.max().item())
    fns = {}
    if stored:
        fns["stored"] = lambda: _lib.check(H.lib.gpimhip_ivr_exact(*head(H), *out))
    for b in bands:
        fns["band%d" % b] = lambda b=b: _lib.check(H.lib.gpimhip_ivr_exact_banded(*head(H), b, *out))
    for k, (med, lo) in timed(fns, reps).items():
        res[k + "_ms"], res[k + "_min_ms"] = med, lo
    if stored:
        res["acq_max_stored"] = float(acq.max().item())
    if q:
        gf = {}
        if stored:
            gf["greedy_stored"] = lambda: _lib.check(H.lib.gpimhip_ivr_greedy(*head(H), *gout))
        gb = max(b for b in bands if b <= 32) if any(b <= 32 for b in bands) else min(bands)
        gf["greedy_band%d" % gb] = lambda: _lib.check(H.lib.gpimhip_ivr_greedy_banded(*head(H), gb, *gout))
        for k, (med, lo) in timed(gf, reps).items():
            res[k + "_ms"], res[k + "_min_ms"] = med, lo
            res[k + "_picks"] = idx.tolist()
    nb = (N + 127) // 128
    res["tn_flop"] = 2.0 * (nt * (nt + 1) // 2) * 128 * 128 * nb * 128
    res["workspace_bytes_all"] = int(H.lib.gpimhip_workspace_bytes(H.h))
    H.close()
    Hb.close()
    return res


if __name__ == "__main__":
    if "--profile" in sys.argv:
        i = sys.argv.index("--profile")
        print(json.dumps(run(int(sys.argv[i + 1]), int(sys.argv[i + 2]), (32,), reps=3, q=0)), flush=True)
    elif "--big" in sys.argv:
        N, M = 4212, 65536
        print(json.dumps(run(N, M, (_ivr_band("auto", M),), q=0, stored=False)), flush=True)
    else:
        for N, M in ((1024, 4096), (4212, 16384)):
            print(json.dumps(run(N, M, (8, 32, (M + 127) // 128))), flush=True)
