"""Times gpimhip_ivr_greedy calls of q = 1, 10 and 32 picks next to one gpimhip_ivr_exact call of the same model and grid
(DESIGN.md section 27): a warm handle, a host clock around a call that ends in the entry's synchronise, the median of 10
calls, (N, M) = (1024, 4096) and (4212, 16384), the problems of tests/tools/bench_ivr.py; one JSON line per case, with the
bytes one fused pass moves (every stored entry of C read once and written once) for the achieved rate from a kernel trace.
`--profile N M`: three calls of q = 10 and three gpimhip_ivr_exact calls at (N, M) only, for a run of its own under
`rocprofv3 --kernel-trace --stats`: colsq_sym_kernel<false> in the same trace is the read-only yardstick of the pass."""
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


def run(N, M, qs=QS, reps=10):
    spec, u, X, y, G = problem(N, M)
    m = spec.struct()
    H = _lib.Handle()
    qmax = max(qs)
    mean, sd, acq, after = (torch.empty(M, dtype=torch.float64, device="cuda") for _ in range(4))
    maps = torch.empty((qmax, M), dtype=torch.float64, device="cuda")
    gain = torch.empty(qmax, dtype=torch.float64, device="cuda")
    idx = torch.empty(qmax, dtype=torch.int64, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    head = (H.h, ctypes.byref(m), _lib.ptr(X), _lib.ptr(y), N, _lib.ptr(u), _lib.ptr(G), M, None, None)
    ivr = lambda: _lib.check(H.lib.gpimhip_ivr_exact(*head, _lib.ptr(mean), _lib.ptr(sd), _lib.ptr(acq)))
    greedy = lambda q: (lambda: _lib.check(H.lib.gpimhip_ivr_greedy(*head, q, _lib.ptr(mean), _lib.ptr(sd), _lib.ptr(maps),
                                                                    _lib.ptr(after), _lib.ptr(idx), _lib.ptr(gain),
                                                                    _lib.ptr(count))))
    res = {"N": N, "M": M}
    for name, fn in [("ivr", ivr)] + [("greedy_q%d" % q, greedy(q)) for q in qs] + [("ivr_again", ivr)]:
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
        if name.startswith("greedy"):
            assert int(count.item()) == int(name[8:])
    q = max(qs)
    res["picks"] = idx[:min(q, 10)].tolist()
    res["gain_first_last"] = [float(gain[0].item()), float(gain[q - 1].item())]
    res["acq_max"] = float(acq.max().item())
    nt = (M + 127) // 128
    # stored tiles of C, the upper halves of the diagonal tiles' 32-column groups skipped (ivr.hip: colsq_sym_kernel)
    stored = 8 * (nt * (nt - 1) // 2 * 128 * 128 + nt * sum(32 for rr in range(8) for cc in range(4) if 16 * rr + 15 >= 32 * cc) * 16)
    res["colsq_sym_bytes"] = stored
    res["fused_pass_bytes"] = 2 * stored
    res["workspace_bytes"] = int(H.lib.gpimhip_workspace_bytes(H.h))
    H.close()
    return res


if __name__ == "__main__":
    if "--profile" in sys.argv:
        i = sys.argv.index("--profile")
        print(json.dumps(run(int(sys.argv[i + 1]), int(sys.argv[i + 2]), qs=(10,), reps=1)), flush=True)
        sys.exit(0)
    for N, M in ((1024, 4096), (4212, 16384)):
        print(json.dumps(run(N, M)), flush=True)
