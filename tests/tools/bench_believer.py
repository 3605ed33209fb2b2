"""Times gpimhip_acquire_batch calls (EI) of q = 1, 10 and 32 picks next to one gpimhip_acquire_exact call of the same model
and grid: a warm handle, a host clock around a call that ends in the entry's synchronise, the median
of 10 calls, (N, M) = (1024, 4096), (4212, 16384) and (4212, 65536) -- the last a grid whose posterior covariance would take
32 GiB -- on the problems of tests/tools/bench_ivr.py; one JSON line per case, with the per-further-pick increment and the
bytes one pass over W moves (np x M_pad doubles) for the achieved rate from a kernel trace.
`--profile N M`: three calls of q = 10 and three gpimhip_acquire_exact calls at (N, M) only, for a run of its own under
`rocprofv3 --kernel-trace --stats`: gemv_t_kernel<double> over the K* slab in the same trace streams the same bytes and is
the yardstick of believer_col_kernel."""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from gpim_amd import _lib
from bench_ivr import problem

QS = (1, 10, 32)


def run(N, M, qs=QS, reps=10, kind="ei"):
    spec, u, X, y, G = problem(N, M)
    m = spec.struct()
    H = _lib.Handle()
    qmax = max(qs)
    mean, sd, acq, after = (torch.empty(M, dtype=torch.float64, device="cuda") for _ in range(4))
    maps = torch.empty((qmax, M), dtype=torch.float64, device="cuda")
    val = torch.empty(qmax, dtype=torch.float64, device="cuda")
    idx = torch.empty(qmax, dtype=torch.int64, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    head = (H.h, ctypes.byref(m), _lib.ptr(X), _lib.ptr(y), N, _lib.ptr(u), _lib.ptr(G), M, _lib.ptr(X), N,
            _lib.ACQ_IDS[kind], 0.0, 0.01, None)
    single = lambda: _lib.check(H.lib.gpimhip_acquire_exact(*head, _lib.ptr(mean), _lib.ptr(sd), _lib.ptr(acq)))
    batch = lambda q: (lambda: _lib.check(H.lib.gpimhip_acquire_batch(*head, q, _lib.ptr(mean), _lib.ptr(sd), _lib.ptr(maps),
                                                                      _lib.ptr(after), _lib.ptr(idx), _lib.ptr(val),
                                                                      _lib.ptr(count))))
    res = {"N": N, "M": M, "kind": kind}
    for name, fn in [("acquire_exact", single)] + [("believer_q%d" % q, batch(q)) for q in qs] + [("acquire_exact_again", single)]:
        fn()
        fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()                                    # (the entry synchronises its stream before it returns)
            ts.append(time.perf_counter() - t0)
        res[name + "_ms"] = 1e3 * statistics.median(ts)
        res[name + "_min_ms"] = 1e3 * min(ts)
        if name.startswith("believer"):
            assert int(count.item()) == int(name[10:])
    if len(qs) > 1:
        lo, hi = sorted(qs)[-2:]
        res["per_further_pick_ms"] = (res["believer_q%d_ms" % hi] - res["believer_q%d_ms" % lo]) / (hi - lo)
    q = max(qs)
    res["picks"] = idx[:min(q, 10)].tolist()
    res["val_first_last"] = [float(val[0].item()), float(val[q - 1].item())]
    np_, mp = (N + 127) // 128 * 128, (M + 127) // 128 * 128
    res["pass_bytes"] = 8 * np_ * mp
    res["workspace_bytes"] = int(H.lib.gpimhip_workspace_bytes(H.h))
    H.close()
    return res


if __name__ == "__main__":
    if "--profile" in sys.argv:
        i = sys.argv.index("--profile")
        print(json.dumps(run(int(sys.argv[i + 1]), int(sys.argv[i + 2]), qs=(10,), reps=1)), flush=True)
        sys.exit(0)
    for N, M in ((1024, 4096), (4212, 16384), (4212, 65536)):
        print(json.dumps(run(N, M)), flush=True)
