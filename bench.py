#!/usr/bin/env python
"""
bench.py -- GP fit + predict throughput of the exact-GP hot path on MI355X.

Headline workload (BASELINE.json configs[1], made concrete in SURVEY 8(d) "Config 2"): a synthetic
256x256 twisted-bilayer lattice image, 25 % of the pixels observed (N = 16384 training points,
M = 65536 grid points, d = 2), Matern52 kernel, lengthscale bounds [[1,1],[20,20]], lr 0.1,
T = 100 Adam iterations, fp64, exact GP.  One STEP = one complete reconstructor fit + predict
(the work of ``gpim_amd.reconstructor(...).run()``) with the inputs already resident in HBM and
the hyper-parameters reset to their seeded initial draw, so every step does identical work.

metric  : "GP fit+predict grid-points/sec" = (M * steps * n_gpus) / wall time; the second half of
          BASELINE.json's metric ("posterior RMSE vs reference") is emitted as ``rmse_vs_oracle``
          (config C1 twin, HIP engine vs the CPU oracle on the same inputs).
N > 1   : one process per GPU (torchrun contract).
          --workload c2 (default): every rank reconstructs its own image of a stack (seed = rank) --
              independent units, no collective on the data path -- and the (mean, sd) maps are gathered
              to rank 0 over RCCL inside the timed region.  Weak scaling.
          --workload c1: config C1 as the reference defines it -- the 128x128 PFM spiral scan of
              expdata/spiral_s_00010_2019.npy (committed data fixture, N = 4212, M = 16384), RBF, T = 300 --
              one image per GPU, same step and gather as c2.  Weak scaling.
          --workload c3: the 64 spectral slices of ONE 64x64x64 cube (config C3) are dealt to the ranks
              and fitted in lock-step batches per GPU; total work fixed.  Strong scaling.
          c1 and c3 carry the same ``roofline.stages`` breakdown as c2 (collected in one extra, untimed step with
          the stage timers on, so that the timed steps run the hipGraph-replayed path a user gets) plus
          ``chain_us_per_128`` = Cholesky time per 128-column block step.
          --workload c3cube: the COMPLETE 64x64x64 cube of config C3 as ONE exact GP (N = 262144, Matern52) through the
              reflection symmetry of the grid: eight dense blocks of 32768 points that share only the hyper-parameters,
              dealt to the ranks (gpim_amd/dist_symm.py) -- no data-path collective, one all-reduce of eleven doubles per
              Adam iteration and one of 2 M doubles for the posterior.  Step = 3 Adam iterations + posterior mean and sd at
              all grid points.  Strong scaling.  (One GPU: 193 GiB.)
          --workload c2full: the COMPLETE 256x256 image of config C2 as ONE exact GP (N = 65536, a 32 GiB
              covariance) across the GPUs: block-column-cyclic Cholesky with one panel broadcast per 512
              columns (gpim_amd/dist_chol.py), distributed solves, posterior mean and sd on the grid, at
              fixed hyper-parameters.  Strong scaling.
roofline: fp64 MFMA.  Top level = algorithmic flop of one step (T*N^3 for the fits: potrf N^3/3 +
          L^-1 N^3/3 + K^-1 N^3/3 per Adam iteration; 2N^3/3 + N^2*M for the prediction) / step time
          / 78.6 TFLOP/s.  ``stages`` breaks it down by the blocked-algorithm stage, each timed live
          with HIP events on the engine's stream; ``dominant_launch`` is the one stage that is exactly
          ONE kernel launch (K^-1 = L^-T L^-1), whose average duration is what the rocprofv3 kernel
          trace under profiles/ reports for the same command.
--full  : a plain run sets up, warms up, times the steps and prints the line with the whole-step roofline.  --full adds
          everything below: the extra stage-timer step (roofline.stages, chain_us_per_128, dominant_launch), and on one GPU
          the CPU baseline, rmse_vs_oracle_headline (c2), rmse_vs_oracle and extra (c2, in a child process).
--dump-outputs DIR: after the timed steps, rank 0 writes what the last one computed as DIR/<name>.npy (float64): mean and
          sd (c1 / c2 on the grid, with the hyper-parameter history of rank 0's training; c3, c2full, c3cube likewise).
          The inputs are seeded, so equal arguments give equal inputs from run to run.
cpu_baseline: the CPU oracle (torch fp64 + autograd restatement of the reference, kind "port")
          timed on rank 0's host cores AT THE FULL SIZE of the workload: one Adam iteration (loss + backward +
          step) and one prediction, value = M / (T * t_iteration + t_predict).  Two smaller sizes are timed
          too and fitted to a*N^2 + b*N^3 (resp. c*N*M + e*N^2*M) as a cross-check of the measurement.
extra   : driver-run throughputs of the other BASELINE.json configs (C1, C3, C4, C5) on one GPU.
"""
import argparse
import ctypes
import json
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FP64_MFMA_PEAK_TFLOPS = 78.6      # MI355X fp64 matrix peak (vendor spec; = vector fp64 rate)

WORKLOAD = dict(size=256, frac=0.25, kernel="Matern52", lengthscale=[[1., 1.], [20., 20.]],
                learning_rate=0.1, iterations=100)
C1 = dict(kernel="RBF", lengthscale=[[1., 1.], [4., 4.]], learning_rate=0.1, iterations=300)
C3 = dict(kernel="RBF", lengthscale=[[1., 1.], [20., 20.]], learning_rate=0.1, iterations=250)


# ------------------------------------------------------------------------------------------------
# CPU baseline (oracle on the host cores)
# ------------------------------------------------------------------------------------------------
def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(N, M, T, workload=None, full=True):
    """Times the oracle (a) at the FULL size of the workload -- one Adam iteration (loss + backward + step;
    every iteration does the same work) and one prediction on all M grid points -- and (b) at N ~ 2048 and
    4096 of the same workload, fitted to  t_iter(N) = a N^2 + b N^3,  t_pred(N, M) = c N M + e N^2 M  and
    evaluated at the full size as a cross-check.  value = M / (T * t_iter + t_pred) from (a)."""
    from oracle import gpim_oracle as O
    from problems import lattice_image
    W = workload or WORKLOAD
    # LAPACK/BLAS on this path stop scaling (and oversubscribe badly) far below the 100+ hardware
    # threads of a GPU host; 32 threads is where the oracle's iteration time bottoms out
    threads = min(os.cpu_count() or 1, 32)
    torch.set_num_threads(threads)

    kept = {}

    def sample(n, iters, predict, keep=False):
        size = int(round(math.sqrt(n / W["frac"])))
        R, _ = lattice_image(size=size, frac=W["frac"], seed=1)
        X, Xf = O.get_sparse_grid(R), O.get_full_grid(R)
        rec = O.reconstructor(X, R, Xf, kernel=W["kernel"], lengthscale=W["lengthscale"],
                              learning_rate=W["learning_rate"], iterations=iters, verbose=0)
        t0 = time.time()
        rec.train()
        t_it = (time.time() - t0) / iters
        t_pr = None
        if predict:
            t0 = time.time()
            mean, sd = rec.predict()
            t_pr = time.time() - t0
            if keep:
                # what the timed oracle run computed: the posterior after `iters` Adam iterations from the seeded draw
                # and the hyper-parameter history -- the headline parity check compares the engine with it
                kept.update(mean=np.asarray(mean), sd=np.asarray(sd), iterations=iters,
                            hyper={k: np.asarray(v) for k, v in rec.hyperparams.items()})
        return rec.X.shape[0], size * size, t_it, t_pr

    sample(256, 1, True)                          # thread-pool / allocator warm-up, not timed
    pts = [sample(2048, 2, True), sample(4096, 2, True)]
    n_ = np.array([p[0] for p in pts], dtype=float)
    m_ = np.array([p[1] for p in pts], dtype=float)
    t_it = np.array([p[2] for p in pts])
    t_pr = np.array([p[3] for p in pts])

    def nnls2(A, y):
        # two-term non-negative least squares in relative error (every sample weighs the same)
        Aw, yw = A / y[:, None], np.ones_like(y)
        best = None
        for cols in ([0, 1], [1], [0]):
            c, *_ = np.linalg.lstsq(Aw[:, cols], yw, rcond=None)
            if (c >= 0).all():
                full_c = np.zeros(2)
                full_c[cols] = c
                res = float(np.sqrt(np.mean((Aw @ full_c - 1.0) ** 2)))
                if best is None or res < best[1]:
                    best = (full_c, res)
        return best

    (a, b), _ = nnls2(np.stack([n_ ** 2, n_ ** 3], 1), t_it)
    (c, e), _ = nnls2(np.stack([n_ * m_, n_ ** 2 * m_], 1), t_pr)
    fit_iter, fit_pred = a * N ** 2 + b * N ** 3, c * N * M + e * N ** 2 * M
    # (a) the measurement.  The oracle's predict holds K*, L^-1 K* and its square (3 x 8 N M bytes) plus K and L.
    need = 3 * 8.0 * N * M + 6 * 8.0 * N * N
    try:
        import psutil
        avail = psutil.virtual_memory().available
    except Exception:
        avail = None
    measured = full and (avail is None or avail > 1.3 * need)
    if measured:
        n_full, m_full, t_iter_full, t_pred_full = sample(N, 1, True, keep=True)
        assert n_full == N and m_full == M, (n_full, m_full)
    else:
        t_iter_full, t_pred_full = fit_iter, fit_pred
    t_full = T * t_iter_full + t_pred_full
    text = ("oracle (torch CPU fp64, autograd), %d threads on '%s' (os.cpu_count() = %s); %s at N=%d, M=%d: "
            "%.1f s per Adam iteration (1 timed), %.1f s per prediction (1 timed); whole job = T=%d iterations + 1 "
            "prediction; cross-check from samples (N, M, s/iteration, s/predict) %s fitted to a N^2 + b N^3 and "
            "c N M + e N^2 M: %.1f s / %.1f s"
            % (threads, _cpu_model(), os.cpu_count(), "MEASURED" if measured else "NOT measured (host memory), fit evaluated",
               N, M, t_iter_full, t_pred_full, T,
               [(int(p[0]), int(p[1]), round(p[2], 3), round(p[3], 3)) for p in pts], fit_iter, fit_pred))
    return {"_oracle_full": kept or None,
            "value": M / t_full, "unit": "grid-points/s", "cores": threads, "kind": "port", "sample": text,
            "measured_at_full_size": bool(measured), "cpu_model": _cpu_model(), "os_cpu_count": os.cpu_count(),
            "torch_num_threads": torch.get_num_threads(),
            "s_per_iteration_full": t_iter_full, "s_per_predict_full": t_pred_full,
            "fit_cross_check": {"t_iter": {"N2": a, "N3": b, "at_full_size": fit_iter},
                                "t_pred": {"NM": c, "N2M": e, "at_full_size": fit_pred}}}


def cpu_baseline_c1(R, T):
    """Config C1 on the host cores: 3 oracle Adam iterations + 1 prediction at the full size (N = 4212, M = 16384);
    value = M / (T * t_iteration + t_predict)."""
    from oracle import gpim_oracle as O
    threads = min(os.cpu_count() or 1, 32)
    torch.set_num_threads(threads)
    X, Xf = O.get_sparse_grid(R), O.get_full_grid(R)
    O.reconstructor(X, R, Xf, **dict(C1, iterations=1, verbose=0)).train()             # warm-up
    rec = O.reconstructor(X, R, Xf, **dict(C1, iterations=3, verbose=0))
    t0 = time.time(); rec.train(); t_it = (time.time() - t0) / 3
    t0 = time.time(); rec.predict(); t_pr = time.time() - t0
    return {"value": R.size / (T * t_it + t_pr), "unit": "grid-points/s", "cores": threads, "kind": "port",
            "measured_at_full_size": True, "cpu_model": _cpu_model(), "os_cpu_count": os.cpu_count(),
            "torch_num_threads": torch.get_num_threads(), "s_per_iteration_full": t_it, "s_per_predict_full": t_pr,
            "sample": "oracle, %d threads: 3 Adam iterations (%.2f s each) + 1 prediction (%.2f s) at N=%d, M=%d; whole job "
                      "= T=%d iterations + 1 prediction" % (threads, t_it, t_pr, int(np.isfinite(R).sum()), R.size, T)}


# ------------------------------------------------------------------------------------------------
# the other half of the metric: posterior RMSE vs the reference restatement
# ------------------------------------------------------------------------------------------------
def rmse_vs_oracle(gpim, iterations=5):
    """Config C1 (the reference's 128x128 PFM spiral scan, N = 4212, M = 16384, RBF): HIP engine vs oracle, same
    inputs, same seed, `iterations` Adam steps (the oracle needs ~1 s per step on the host)."""
    from oracle import gpim_oracle as O
    from problems import spiral_pfm_image
    R = spiral_pfm_image()
    X, Xf = gpim.utils.get_sparse_grid(R), gpim.utils.get_full_grid(R)
    kw = dict(C1, iterations=iterations, verbose=0)
    mean, sd, hyper = gpim.reconstructor(X, R, Xf, **kw).run()
    torch.set_num_threads(min(os.cpu_count() or 1, 32))
    mo, so, ho = O.reconstructor(X, R, Xf, **kw).run()
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))))
    return {"config": "C1: 128x128 PFM spiral scan (expdata/spiral_s_00010_2019.npy), N=%d, M=%d, RBF, %d Adam its, fp64"
                      % (np.isfinite(R).sum(), R.size, iterations),
            "rmse_mean": float(np.sqrt(np.mean((mean - mo) ** 2))),
            "rmse_sd": float(np.sqrt(np.mean((sd - so) ** 2))),
            "max_abs_mean": float(np.max(np.abs(mean - mo))), "max_abs_sd": float(np.max(np.abs(sd - so))),
            "hyperparams_max_rel": max(rel(hyper["lengthscale"], ho["lengthscale"]), rel(hyper["noise"], ho["noise"]),
                                       rel(hyper["variance"], ho["variance"]))}


def rmse_vs_oracle_c3(cube, iterations=5, slices=(0, 31, 63)):
    """Config C3 at its own size (64x64x64 twin: N = 1207 per slice -- ragged last block, nb = 10 -- M = 4096, RBF):
    three slices out of dist.reconstruct_slices (lock-step batch of 64 AND batch='auto') against the oracle's
    per-slice reconstructor, `iterations` Adam steps."""
    from oracle import gpim_oracle as O
    from gpim_amd import dist as gdist
    import gpim_amd as gpim
    kw = dict(C3, iterations=iterations)
    res = {"config": "C3: 64x64x64 cube twin, slices %s, N=%d, M=%d, RBF, %d Adam its, fp64"
                     % (list(slices), int(np.isfinite(cube[..., 0]).sum()), cube[..., 0].size, iterations)}
    torch.set_num_threads(min(os.cpu_count() or 1, 32))
    orc = {}
    for k in slices:
        R = cube[..., k]
        orc[k] = O.reconstructor(gpim.utils.get_sparse_grid(R), R, gpim.utils.get_full_grid(R), verbose=0, **kw).run()
    for name, bkw in (("batch64", dict(batch=64)), ("auto", dict(batch="auto"))):
        mean, sd, hyper = gdist.reconstruct_slices(cube, axis=-1, return_hyperparams=True, **bkw, **kw)
        em = np.concatenate([(mean[..., k] - orc[k][0]).ravel() for k in slices])
        es = np.concatenate([(sd[..., k] - orc[k][1]).ravel() for k in slices])
        hrel = 0.0
        for k in slices:
            ho = orc[k][2]
            href = np.column_stack([np.reshape(ho["variance"], (iterations, -1)), np.reshape(ho["lengthscale"], (iterations, -1)),
                                    np.reshape(ho["noise"], (iterations, -1))])
            hrel = max(hrel, float(np.max(np.abs(hyper[k] - href) / np.abs(href))))
        res[name] = {"rmse_mean": float(np.sqrt(np.mean(em ** 2))), "rmse_sd": float(np.sqrt(np.mean(es ** 2))),
                     "max_abs_mean": float(np.max(np.abs(em))), "max_abs_sd": float(np.max(np.abs(es))),
                     "hyperparams_max_rel": hrel}
    return res


# ------------------------------------------------------------------------------------------------
# per-stage rooflines from the library's HIP-event stage timers
# ------------------------------------------------------------------------------------------------
STAGE_NAMES = ["potrf", "trtri", "lauum", "predict_var"]


def timers_clear(lib, h):
    tot, cnt = ctypes.c_double(), ctypes.c_int64()
    for s in range(4):
        lib.gpimhip_timing_read(h, s, ctypes.byref(tot), ctypes.byref(cnt))


def timers_read(lib, h):
    tot, cnt = ctypes.c_double(), ctypes.c_int64()
    out = {}
    for s, name in enumerate(STAGE_NAMES):
        lib.gpimhip_timing_read(h, s, ctypes.byref(tot), ctypes.byref(cnt))
        out[name] = (tot.value, cnt.value)
    return out


def stage_breakdown(stage_ms, n_obs, nprob_, M, ms_step, stage_steps):
    """roofline.stages from the HIP-event stage timers: per blocked-algorithm stage the calls, ms per call,
    flop per call (all `nprob_` problems of a lock-step batch), TFLOP/s, fraction of the fp64 MFMA peak and
    share of the time of the step(s) the timers covered."""
    n3 = float(n_obs) ** 3 * nprob_
    # The triangular inverse rides in the launches of the factorisation (cholstep.hip: plan_inverse); the two
    # timers are "the step launches" (timer 0) and "what is left of the inverse afterwards" (timer 1), so the
    # stage that can be priced is their sum: 2 N^3 / 3 flop.
    pm, pn = stage_ms["potrf"]
    tm, tn = stage_ms["trtri"]
    per_call = {"factor_inverse": 2 * n3 / 3, "lauum": n3 / 3}
    label = {"factor_inverse": "potrf + trtri (L^-1 in one pass: inverse tiles hosted by the factorisation's launches)",
             "lauum": "lauum (K^-1 = L^-T L^-1)", "predict_var": "predict_var (L^-1 K*)"}
    stage_ms_ = dict(stage_ms, factor_inverse=(pm + tm, pn))
    stages = []
    for name in ("factor_inverse", "lauum", "predict_var"):
        ms, n = stage_ms_[name]
        if not n:
            continue
        # predict_var: one launch per slab of test points, N^2*M flop per problem over all slabs of a step
        fl = per_call.get(name, float(n_obs) ** 2 * M * nprob_ * stage_steps / n)
        tf = fl / (ms / n * 1e-3) / 1e12
        stages.append({"stage": label[name], "calls": n, "ms_per_call": ms / n, "flop_per_call": fl,
                       "tflops": tf, "frac": tf / FP64_MFMA_PEAK_TFLOPS,
                       "share_of_step": ms / (ms_step * stage_steps)})
        if name == "factor_inverse":
            stages[-1]["ms_step_launches"] = pm / pn
            stages[-1]["ms_after_last_step"] = tm / pn
    return stages


def chain_us(stage_ms, n_obs):
    """time of the factorisation's step launches per 128-column block step"""
    pm, pn = stage_ms["potrf"]
    return (pm / pn * 1e3 / math.ceil(n_obs / 128.0)) if pn else None


# ------------------------------------------------------------------------------------------------
# the other single-GPU configs (driver-verified throughputs for DESIGN.md section 4)
# ------------------------------------------------------------------------------------------------
def _settle_interpreter():
    """A full pass of CPython's cyclic collector over this process's heap (torch, numpy, the oracle's modules) takes 35-170 ms
    and finds nothing; when one falls into a timed region of a few hundred milliseconds (C4: 0.285 s) it reads as a 15-60 %
    slower engine (tools/r5_c4_gc.py).  Collect now and move what survives to the permanent generation, so that the timed
    regions below see collections of their own garbage only."""
    import gc
    gc.collect()
    gc.freeze()


def c4_against_oracle(bo):
    """The timed C4 instance itself (README.md:71-106 of the reference: 25x25, np.random.seed(42), 4 seed points, EI,
    30 exploration steps x 1000 Adam iterations) against the oracle's boptimizer on the host: the sequence of queried
    indices must be EQUAL, the hyper-parameters after every training agree to `hyper_max_rel`."""
    from oracle import gpim_oracle as O
    from problems import notebook_problem
    torch.set_num_threads(min(os.cpu_count() or 1, 8))
    trial_func, Z = notebook_problem(4)
    tmp = tempfile.mkdtemp()
    t0 = time.perf_counter()
    ob = O.boptimizer(O.get_sparse_grid(Z), Z, O.get_full_grid(Z), trial_func, acquisition_function="ei",
                      exploration_steps=30, verbose=0, filename=os.path.join(tmp, "bo_oracle"))
    ob.run()
    t_orc = time.perf_counter() - t0
    ih, io = [tuple(int(v) for v in i) for i in bo.indices_all], [tuple(int(v) for v in i) for i in ob.indices_all]
    hh, ho = bo.surrogate_model.hyperparams, ob.surrogate_model.hyperparams
    out = {"indices_equal_oracle": ih == io, "n_queries": len(ih), "oracle_seconds": t_orc,
           "oracle": "oracle boptimizer (torch CPU fp64) on the same instance, same seed; every one of the 31 x 1000 "
                     "hyper-parameter rows compared.  With a handful of points the noise parameter sits on a flat direction "
                     "and Adam turns rounding-size gradient differences into visibly different steps of THAT training, which "
                     "then rejoins the other trajectory (the queried points do not change): hence the three figures per "
                     "parameter -- worst row, fraction of rows within 1e-7, worst end-of-training row"}
    rel_all = 0.0
    for key in ("variance", "lengthscale", "noise"):
        a, b = np.asarray(hh[key], dtype=float), np.asarray(ho[key], dtype=float)
        if a.shape != b.shape or a.shape[0] % 1000:
            out["hyper_max_rel"] = float("inf")
            return out
        rel = (np.abs(a - b) / np.abs(b)).reshape(a.shape[0], -1).max(axis=1)
        out["hyper_" + key] = {"max_rel": float(rel.max()), "rows_within_1e-7": float((rel <= 1e-7).mean()),
                               "first_3_trainings_max_rel": float(rel[:3000].max()),
                               "end_of_training_max_rel": float(rel.reshape(-1, 1000)[:, -1].max())}
        if key != "noise":
            rel_all = max(rel_all, float(rel.max()))
    out["hyper_max_rel"] = rel_all                    # variance and lengthscale (the noise parameter: see "oracle")
    out["hyper_rows_compared"] = int(np.asarray(hh["noise"]).shape[0])
    return out


def extra_configs(gpim):
    from gpim_amd import dist as gdist
    from problems import ckpfm_cube, hyperspectral_cube, notebook_problem, spiral_pfm_image
    out = {}
    sync = torch.cuda.synchronize
    _settle_interpreter()
    # C1: the reference's 128x128 PFM spiral scan, RBF, T = 300
    R = spiral_pfm_image()
    X, Xf = gpim.utils.get_sparse_grid(R), gpim.utils.get_full_grid(R)
    gpim.reconstructor(X, R, Xf, **dict(C1, iterations=3, verbose=0)).run()          # workspace / plan warm-up
    sync(); t0 = time.perf_counter()
    rec1 = gpim.reconstructor(X, R, Xf, verbose=0, **C1)
    rec1.run()
    sync(); dt = time.perf_counter() - t0
    n1 = int(np.isfinite(R).sum())
    flop1 = 300 * float(n1) ** 3 + 2 * float(n1) ** 3 / 3 + float(n1) ** 2 * R.size
    out["C1"] = {"workload": "128x128 PFM spiral scan (expdata/spiral_s_00010_2019.npy), N=%d, M=%d, RBF, T=300, "
                             "reconstructor.run()" % (n1, R.size),
                 "seconds": dt, "grid_points_per_s": R.size / dt, "ms_per_adam_iteration": dt / 300 * 1e3,
                 "mfma_frac": flop1 / dt / 1e12 / FP64_MFMA_PEAK_TFLOPS}
    # per-stage rooflines of C1: one more (untimed) fit + predict on the same object with the stage timers on
    lib1, h1 = rec1._handle.lib, rec1._handle.h
    lib1.gpimhip_timing_enable(h1, 1)
    timers_clear(lib1, h1)
    sync(); t0 = time.perf_counter()
    rec1.train()
    rec1.predict()
    sync(); dts = time.perf_counter() - t0
    lib1.gpimhip_timing_enable(h1, 0)
    sm1 = timers_read(lib1, h1)
    out["C1"]["roofline"] = {"bound": "mfma", "achieved": flop1 / dt / 1e12, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                             "frac": out["C1"]["mfma_frac"],
                             "stages": stage_breakdown(sm1, n1, 1, R.size, dts * 1e3, 1),
                             "stages_from": "one extra fit + predict after the timed one, stage timers on (%.1f ms: launch by "
                                            "launch, the timed run replays a captured iteration)" % (dts * 1e3),
                             "chain_us_per_128": chain_us(sm1, n1)}
    del rec1
    # C3: 64 slices of 64x64, RBF, T = 250: four lock-step batches of 16 at a time on one GPU
    cube, _ = hyperspectral_cube()
    gdist.reconstruct_slices(cube, axis=-1, batch=16, batch_concurrency=4, **dict(C3, iterations=3))
    sync(); t0 = time.perf_counter()
    gdist.reconstruct_slices(cube, axis=-1, batch=16, batch_concurrency=4, **C3)
    sync(); dt = time.perf_counter() - t0
    n3_ = int(np.isfinite(cube[..., 0]).sum())
    flop3 = 64 * (250 * float(n3_) ** 3 + 2 * float(n3_) ** 3 / 3 + float(n3_) ** 2 * 4096)
    out["C3"] = {"workload": "64x64x64 cube twin, 64 per-slice GPs (N=%d, M=4096), RBF, T=250, "
                             "dist.reconstruct_slices(batch=16, batch_concurrency=4) on one GPU" % n3_,
                 "seconds": dt, "grid_points_per_s": cube.size / dt, "mfma_frac": flop3 / dt / 1e12 / FP64_MFMA_PEAK_TFLOPS}
    # per-stage rooflines of C3: one more (untimed) step with all 64 slices as ONE lock-step batch on one handle and the
    # stage timers on (the timers need one handle and stream; share_of_step is relative to that serial step)
    from gpim_amd import _lib as _l
    H3 = _l.Handle()
    gdist.reconstruct_slices(cube, axis=-1, batch=64, handle=H3, **dict(C3, iterations=2))
    H3.lib.gpimhip_timing_enable(H3.h, 1)
    timers_clear(H3.lib, H3.h)
    sync(); t0 = time.perf_counter()
    gdist.reconstruct_slices(cube, axis=-1, batch=64, handle=H3, **C3)
    sync(); dts = time.perf_counter() - t0
    H3.lib.gpimhip_timing_enable(H3.h, 0)
    sm3 = timers_read(H3.lib, H3.h)
    out["C3"]["roofline"] = {"bound": "mfma", "achieved": flop3 / dt / 1e12, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                             "frac": out["C3"]["mfma_frac"],
                             "stages": stage_breakdown(sm3, n3_, 64, 4096, dts * 1e3, 1),
                             "stages_from": "one extra step with the 64 slices as ONE lock-step batch per launch, stage timers "
                                            "on (%.1f ms; the timed step runs 4 concurrent batches of 16 and replays captured "
                                            "iterations)" % (dts * 1e3),
                             "chain_us_per_128": chain_us(sm3, n3_)}
    H3.close()
    del H3
    # the per-rank share of C3 on an 8-GPU node: 8 of the 64 slices (round-robin shard of rank 0) on ONE GPU, the
    # batch split dist.reconstruct_slices picks by itself
    sub = cube[..., 0::8]
    gdist.reconstruct_slices(sub, axis=-1, batch="auto", **dict(C3, iterations=3))
    sync(); t0 = time.perf_counter()
    gdist.reconstruct_slices(sub, axis=-1, batch="auto", **C3)
    sync(); dt = time.perf_counter() - t0
    out["C3_per_rank_8"] = {"workload": "rank 0's share of C3 at world size 8: slices 0, 8, ..., 56 of the cube twin on one GPU, "
                                        "RBF, T=250, dist.reconstruct_slices(batch='auto')",
                            "seconds": dt, "grid_points_per_s": sub.size / dt,
                            "projected_8gpu_speedup_over_1gpu": out["C3"]["seconds"] / dt}
    out["rmse_vs_oracle_c3"] = rmse_vs_oracle_c3(cube)
    # C4: BO on 25x25, EI, 30 exploration steps x 1000 Adam iterations (README.md:71-106 of the reference)
    tmp = tempfile.mkdtemp()
    _settle_interpreter()                                                              # (the oracle run above left a large heap)
    for rep in range(2):                                                               # first pass = warm-up
        trial_func, Z = notebook_problem(4)
        bo = gpim.boptimizer(gpim.utils.get_sparse_grid(Z), Z, gpim.utils.get_full_grid(Z), trial_func,
                             acquisition_function="ei", exploration_steps=30, verbose=0,
                             filename=os.path.join(tmp, "bo"))
        sync(); t0 = time.perf_counter()
        bo.run()
        sync(); dt = time.perf_counter() - t0
    out["C4"] = {"workload": "BO 25x25, EI, 30 steps x (1000 Adam its + acquisition sweep), boptimizer.run()",
                 "seconds": dt, "grid_points_per_s": 625 * 30 / dt, "steps_per_s": 30 / dt,
                 "us_per_adam_iteration": dt / (31 * 1000) * 1e6}
    out["C4"].update(c4_against_oracle(bo))
    # C5: 4D cKPFM twin 10x10x64x5, one GP per Ns slice (N = 6400 points in 3-D, fully observed), T = 200:
    # (i) the reference's model for it -- sparse VFE with indpoints=512 (534 inducing inputs);
    # (ii) the same slices as EXACT GPs through the Kronecker solver (possible because the slices are complete grids)
    cube4 = ckpfm_cube()
    kw5 = dict(kernel="RBF", learning_rate=0.05, iterations=200)
    gdist.reconstruct_slices(cube4[..., :1], axis=-1, sparse=True, indpoints=512, **dict(kw5, iterations=3))
    sync(); t0 = time.perf_counter()
    gdist.reconstruct_slices(cube4, axis=-1, sparse=True, indpoints=512, **kw5)
    sync(); dt = time.perf_counter() - t0
    out["C5"] = {"workload": "10x10x64x5 cKPFM twin, 5 per-Ns slices (N=6400 each), sparse VFE with 534 inducing inputs, "
                             "RBF, T=200, dist.reconstruct_slices on one GPU",
                 "seconds": dt, "grid_points_per_s": cube4.size / dt, "ms_per_adam_iteration": dt / (5 * 200) * 1e3}
    R5 = cube4[..., 0]
    Xf5 = gpim.utils.get_full_grid(R5)
    gpim.reconstructor(Xf5, R5, Xf5, structured=True, verbose=0, **dict(kw5, iterations=3)).run()
    sync(); t0 = time.perf_counter()
    for k in range(cube4.shape[-1]):
        gpim.reconstructor(Xf5, cube4[..., k], Xf5, structured=True, verbose=0, **kw5).run()
    sync(); dt = time.perf_counter() - t0
    out["C5_structured_exact"] = {"workload": "the same 5 slices as exact GPs through the Kronecker solver "
                                              "(reconstructor(structured=True)), RBF, T=200",
                                  "seconds": dt, "grid_points_per_s": cube4.size / dt,
                                  "ms_per_adam_iteration": dt / (5 * 200) * 1e3}
    # the COMPLETE 256x256 image (N = M = 65536, Matern52) as one exact GP: the symmetry-reduced structured solver
    # (reconstructor(structured=True): four reflection blocks of 16384 points in one lock-step batch) next to the dense
    # distributed driver on the same GPU (dist_chol.exact_gp_fit, P = 1)
    from problems import lattice_image as _li
    from gpim_amd.dist_chol import exact_gp_fit
    Rc, _ = _li(size=WORKLOAD["size"], frac=1.0, seed=1)
    Xc = gpim.utils.get_full_grid(Rc)
    kwc = dict(kernel=WORKLOAD["kernel"], lengthscale=WORKLOAD["lengthscale"], learning_rate=WORKLOAD["learning_rate"], verbose=0)
    rc_ = gpim.reconstructor(Xc, Rc, Xc, structured=True, iterations=2, **kwc)
    rc_.train()
    sync(); t0 = time.perf_counter()
    rc_.train(iterations=5)
    sync(); t_it = (time.perf_counter() - t0) / 5
    t0 = time.perf_counter()
    rc_.predict()
    sync(); t_pr = time.perf_counter() - t0
    loss_s = list(rc_.loss_all[0:2])
    del rc_
    gc_ = __import__("gc"); gc_.collect(); torch.cuda.empty_cache()
    ii, jj = np.meshgrid(np.arange(Rc.shape[0], dtype=np.float64), np.arange(Rc.shape[1], dtype=np.float64), indexing="ij")
    Xf_, yf_ = np.stack([ii.ravel(), jj.ravel()], 1), Rc.ravel()
    sync(); t0 = time.perf_counter()
    hyp_d, _ = exact_gp_fit(Xf_, yf_, iterations=2, kernel=WORKLOAD["kernel"], lengthscale=WORKLOAD["lengthscale"],
                            learning_rate=WORKLOAD["learning_rate"])
    sync(); t_dense = (time.perf_counter() - t0) / 2
    gc_.collect(); torch.cuda.empty_cache()
    out["C2_complete_structured"] = {
        "workload": "the complete 256x256 image (N = M = 65536), Matern52: reconstructor(structured=True) -- four reflection "
                    "blocks of 16384 points, one lock-step batch with shared hyper-parameters; exact",
        "seconds_per_adam_iteration": t_it, "predict_seconds": t_pr,
        "dense_seconds_per_adam_iteration": t_dense, "speedup_over_dense": t_dense / t_it,
        "loss_first_two_iterations": loss_s, "dense_loss_first_two_iterations": [float(v) for v in hyp_d["loss"][:2]]}
    # C2 in single precision: the headline workload with reconstructor(precision='single') (float matrices, fp32
    # matrix cores; gpimhip_set_precision) -- NOT the headline number, whose dtype is the reference's default f64
    from problems import lattice_image
    import gc
    del bo
    gc.collect()                      # handles of the earlier configs (and their side streams) go away
    R2, _ = lattice_image(size=WORKLOAD["size"], frac=WORKLOAD["frac"], seed=1)
    X2, Xf2 = gpim.utils.get_sparse_grid(R2), gpim.utils.get_full_grid(R2)
    kw2 = dict(kernel=WORKLOAD["kernel"], lengthscale=WORKLOAD["lengthscale"], learning_rate=WORKLOAD["learning_rate"],
               verbose=0, seed=0, precision="single")
    rec2 = gpim.reconstructor(X2.astype(np.float32), R2.astype(np.float32), Xf2.astype(np.float32), iterations=2, **kw2)
    rec2.run()                                                                         # workspace / plan warm-up
    rec2.iterations = WORKLOAD["iterations"]
    sync(); t0 = time.perf_counter()
    rec2.train()
    sync(); t1 = time.perf_counter()
    rec2.predict()
    sync(); dt = time.perf_counter() - t0
    print("C2 single: train %.3f s, predict %.3f s" % (t1 - t0, dt - (t1 - t0)), file=sys.stderr)
    n2, T2 = rec2.X.shape[0], WORKLOAD["iterations"]
    flop2 = T2 * float(n2) ** 3 + 2 * float(n2) ** 3 / 3 + float(n2) ** 2 * R2.size
    out["C2_single_precision"] = {"workload": "the headline workload with precision='single': 256x256, N=%d, M=%d, Matern52, "
                                              "T=%d, fit + predict" % (n2, R2.size, T2),
                                  "dtype": "f32 matrices and MFMA; f64 diagonal blocks, vectors, loss, gradient, Adam",
                                  "seconds": dt, "grid_points_per_s": R2.size / dt, "tflops": flop2 / dt / 1e12,
                                  "mfma_frac_of_fp32_peak": flop2 / dt / 1e12 / 157.3}
    # the complete 64x64x64 cube of config C3 as ONE exact GP (N = 262144; the reference fits whole cubes as one GP,
    # gpr.py:30-43) through the reflection blocks: eight dense blocks of 32768 points in one lock-step batch, 193 GiB of
    # the 288 GB.  Last, and guarded: it needs most of the device's memory.
    try:
        del rec2
        gc.collect(); torch.cuda.empty_cache()
        _, cube_full = hyperspectral_cube()
        Xc3 = gpim.utils.get_full_grid(cube_full)
        rec3 = gpim.reconstructor(Xc3, cube_full, Xc3, structured=True, kernel="Matern52",
                                  lengthscale=[[1., 1., 1.], [20., 20., 20.]], learning_rate=0.1, iterations=1, verbose=0)
        rec3.train()
        sync(); t0 = time.perf_counter()
        rec3.train(iterations=2)
        sync(); dt = (time.perf_counter() - t0) / 2
        n3 = cube_full.size
        out["C3_cube_as_one_GP_structured"] = {
            "workload": "the complete 64x64x64 cube as ONE exact GP (N = %d), Matern52, reconstructor(structured=True): eight "
                        "reflection blocks of %d points, one lock-step batch with shared hyper-parameters; exact" % (n3, n3 // 8),
            "seconds_per_adam_iteration": dt, "blocks_tflops": 8 * float(n3 // 8) ** 3 / dt / 1e12,
            "dense_equivalent_tflops": float(n3) ** 3 / dt / 1e12,
            "workspace_gib": rec3._handle.lib.gpimhip_workspace_bytes(rec3._handle.h) / 2 ** 30,
            "loss": [float(v) for v in rec3.loss_all]}
        del rec3
        gc.collect(); torch.cuda.empty_cache()
    except Exception as e:                      # (a smaller device: report, do not fail the line)
        out["C3_cube_as_one_GP_structured"] = {"error": "%s: %s" % (type(e).__name__, e)}
    return out


# ------------------------------------------------------------------------------------------------
# --dump-outputs: what the last timed step computed, for comparing two builds output for output
# ------------------------------------------------------------------------------------------------
DUMP_LIMIT_BYTES = 64 * 10 ** 6


def step_outputs(workload, res, world, rec, T):
    """The arrays a caller of the timed path receives from one step, by name (rank 0's view)."""
    if workload in ("c2", "c1"):
        # reconstructor.run(): mean and sd on the grid (one image per rank, gathered to rank 0) and the hyper-parameter
        # history of rank 0's training -- its last T rows, i.e. those of the last step
        pred = res.detach().cpu().numpy()
        shape = ((world,) if world > 1 else ()) + tuple(rec.fulldims)
        hp = rec.hyperparams
        out = {"mean": pred[:, 0].reshape(shape), "sd": pred[:, 1].reshape(shape)}
        for k in ("lengthscale", "variance", "noise"):
            out[k] = np.asarray(hp[k][len(hp[k]) - T:], dtype=np.float64)
        return out
    if workload == "c3":
        mean, sd = res
        return {"mean": mean, "sd": sd}
    if workload == "c2full":
        mean, sd, nll = res
        return {"mean": mean, "sd": sd, "nll": np.array([nll])}
    mean, sd, hyp = res                                  # c3cube
    return dict({"mean": mean, "sd": sd}, **{k: hyp[k] for k in ("variance", "lengthscale", "noise", "loss")})


def dump_outputs(path, arrays):
    arrays = {k: np.asarray(v) for k, v in arrays.items()}
    arrays = {k: v.astype(np.float32 if v.dtype == np.float32 else np.float64, copy=False) for k, v in arrays.items()}
    total = sum(v.nbytes for v in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit("--dump-outputs: %d bytes exceed the %d-byte limit" % (total, DUMP_LIMIT_BYTES))
    os.makedirs(path, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(path, k + ".npy"), v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", choices=["c2", "c1", "c3", "c2full", "c3cube"], default="c2")
    ap.add_argument("--iterations", type=int, default=None,
                    help="Adam iterations per step (the named workloads use 100 (c2) / 300 (c1) / 250 (c3))")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline figure does not need: the per-stage roofline step, "
                         "the CPU baseline, the parity checks against the oracle and the other configs (extra)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (rank 0)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip rmse_vs_oracle and the C1/C3/C4 extras")
    ap.add_argument("--extras-only", action="store_true",
                    help="internal: print {rmse_vs_oracle, extra} as one JSON line and exit (run by a --full "
                         "command in a child process, so that a kernel trace of the parent holds the timed "
                         "workload's launches only)")
    args = ap.parse_args()

    import torch.distributed as dist
    import gpim_amd
    from gpim_amd import _lib, dist as gdist
    from problems import hyperspectral_cube, lattice_image, spiral_pfm_image

    if args.extras_only:
        torch.cuda.set_device(0)
        print(json.dumps({"rmse_vs_oracle": rmse_vs_oracle(gpim_amd), "extra": extra_configs(gpim_amd)}))
        return

    rank, world, local_rank = gdist.init_from_env()
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    def fence():
        if world > 1:
            gdist.barrier()
        torch.cuda.synchronize()

    if world > 1:
        # bring the RCCL communicators up outside the timed region even when --warmup 0
        probe = torch.zeros(8, dtype=torch.float64, device=dev)
        gdist.all_gather([torch.empty_like(probe) for _ in range(world)], probe)
        fence()

    stage_ms = {}
    nprob = 1                       # problems advancing together through every launch (c3: the lock-step batch)
    rec = None                      # c2 / c1: the timed reconstructor
    if args.workload in ("c2", "c1"):
        # ---- build this rank's unit and move it to HBM (untimed)
        if args.workload == "c2":
            T = args.iterations or WORKLOAD["iterations"]
            R, _ = lattice_image(size=WORKLOAD["size"], frac=WORKLOAD["frac"], seed=1 + 10 * rank)
            kw = dict(kernel=WORKLOAD["kernel"], lengthscale=WORKLOAD["lengthscale"], learning_rate=WORKLOAD["learning_rate"])
        else:
            T = args.iterations or C1["iterations"]
            R = spiral_pfm_image()                       # every rank: the same scan (a stack of equal frames)
            kw = dict(kernel=C1["kernel"], lengthscale=C1["lengthscale"], learning_rate=C1["learning_rate"])
        X, Xf = gpim_amd.utils.get_sparse_grid(R), gpim_amd.utils.get_full_grid(R)
        rec = gpim_amd.reconstructor(X, R, Xf, iterations=T, verbose=0, seed=0, **kw)
        N, M = rec.X.shape[0], rec.Xtest.shape[0]
        u0 = rec._u.clone()
        lib, h = rec._handle.lib, rec._handle.h
        units_per_step, scaling = M * world, "weak"

        def step():
            rec._u.copy_(u0)
            rec.train()
            rec.predict()
            mean_d, sd_d = rec._last_pred
            if world > 1:
                return gdist.gather_to_root({rank: torch.stack([mean_d, sd_d])}, world, (2, M), device=dev)
            return torch.stack([mean_d, sd_d]).unsqueeze(0)
    elif args.workload == "c3cube":
        from gpim_amd.dist_symm import symm_gp_fit, symm_gp_posterior, symm_shard
        T = args.iterations or 3
        _, cube_full = hyperspectral_cube()
        Xc = gpim_amd.utils.get_full_grid(cube_full)
        pts = Xc.reshape(3, -1).T.copy()
        N = M = cube_full.size
        units_per_step, scaling = M, "strong"
        lib = h = None
        kwc = dict(kernel="Matern52", lengthscale=[[1., 1., 1.], [20., 20., 20.]])

        def step():
            sh = symm_shard(Xc, cube_full, **kwc)               # the rank's blocks: set-up and workspace are part of the step
            hyp, uc = symm_gp_fit(Xc, cube_full, learning_rate=0.1, iterations=T, shard=sh, **kwc)
            mean_c, sd_c = symm_gp_posterior(Xc, cube_full, None, uc, shard=sh, **kwc)
            return mean_c, sd_c, hyp
    elif args.workload == "c2full":
        from gpim_amd.dist_chol import exact_gp_posterior
        T = 0
        R, _ = lattice_image(size=WORKLOAD["size"], frac=1.0, seed=1)
        ii, jj = np.meshgrid(np.arange(R.shape[0], dtype=np.float64), np.arange(R.shape[1], dtype=np.float64), indexing="ij")
        Xall = np.stack([ii.ravel(), jj.ravel()], 1)
        yall = R.ravel()
        N = M = Xall.shape[0]
        units_per_step, scaling = M, "strong"
        lib = h = None
        hyper = dict(kernel="Matern52", lengthscale=[4.0, 4.0], variance=0.05, noise=4e-4)

        def step():
            return exact_gp_posterior(Xall, yall, Xall, **hyper)
    else:
        T = args.iterations or C3["iterations"]
        cube, _ = hyperspectral_cube()
        N, M = int(np.isfinite(cube[..., 0]).sum()), cube.shape[0] * cube.shape[1]
        units_per_step, scaling = cube.size, "strong"
        Hc3 = _lib.Handle()
        lib, h = Hc3.lib, Hc3.h
        nprob = min(64, len(gdist.shard_units(64, rank, world)))

        # timed steps: four lock-step batches of 16 slices at a time, each on its own stream (the latency-bound launches
        # of one batch overlap the tile products of another: 1.11 -> 0.99 s on one GPU); the stage timers need ONE handle
        # and stream, so the extra (untimed) stage step runs the owned slices as one lock-step batch
        def step(stages=False):
            if stages:
                return gdist.reconstruct_slices(cube, axis=-1, batch=64, handle=Hc3, **dict(C3, iterations=T))
            return gdist.reconstruct_slices(cube, axis=-1, batch="auto", **dict(C3, iterations=T))

    for _ in range(args.warmup):
        step()
    _settle_interpreter()          # (a full pass of the cyclic collector inside the timed region is harness time, see there)
    # The timed steps run with the stage timers OFF for every workload: c1 / c3 replay one captured iteration per Adam
    # step (which the timers would switch off), and the headline (c2, enqueued launch by launch) must not carry
    # instrumentation the other lines do not.  The per-stage breakdown (--full) comes from ONE extra step after the timed
    # ones, with the timers on (HIP events on the handle's stream around every stage).
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        res = step()
    fence()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        # before the stage step: that one runs the same reconstructor again
        dump_outputs(args.dump_outputs, step_outputs(args.workload, res, world, rec, T))
    stage_steps = 1
    ms_stage_step = None
    if args.full and lib is not None:
        lib.gpimhip_timing_enable(h, 1)
        timers_clear(lib, h)
        fence()
        t1 = time.perf_counter()
        step(True) if args.workload == "c3" else step()
        fence()
        ms_stage_step = (time.perf_counter() - t1) * 1e3
        lib.gpimhip_timing_enable(h, 0)
        stage_ms = timers_read(lib, h)
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()

    if rank == 0:
        ms_step = elapsed / args.steps * 1e3
        out = {
            "metric": "GP fit+predict grid-points/sec",
            "value": units_per_step * args.steps / elapsed,
            "unit": "grid-points/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_step,
            "higher_is_better": True, "scaling": scaling, "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
        }
        if args.workload in ("c2", "c1"):
            # sanity: the timed output is finite and shaped (units, 2, M)
            assert res.shape == (world, 2, M) and bool(torch.isfinite(res).all())
            if args.workload == "c2":
                out["config"] = {"workload": ("C2: 256x256 synthetic twisted-lattice image, 25%% observed "
                                              "(N=%d, M=%d, d=2), Matern52 exact GP, T=%d Adam its (lr 0.1) + predict; "
                                              "one image per GPU") % (N, M, T),
                                 "N": N, "M": M, "iterations": T, "kernel": WORKLOAD["kernel"]}
            else:
                out["data"] = "reference data file expdata/spiral_s_00010_2019.npy (committed fixture tests/golden/)"
                out["config"] = {"workload": ("C1: 128x128 PFM spiral scan (expdata/spiral_s_00010_2019.npy, background "
                                              "masked as in examples/notebooks/GP_2D3D_images.ipynb: N=%d, M=%d, d=2), RBF "
                                              "exact GP, lengthscale in [1,4], T=%d Adam its (lr 0.1) + predict; one "
                                              "image per GPU") % (N, M, T),
                                 "N": N, "M": M, "iterations": T, "kernel": C1["kernel"]}
            n3 = float(N) ** 3
            flop_step = T * n3 + 2.0 * n3 / 3.0 + float(N) ** 2 * M       # per GPU
            achieved = flop_step / (ms_step * 1e-3) / 1e12
            traffic = None
            pmc = os.path.join(ROOT, "profiles", "pmc_lauum.json")
            traffic_from = None
            if args.workload == "c2" and os.path.exists(pmc):
                traffic = json.load(open(pmc)).get("hbm_bytes_per_launch")
                traffic_from = "profiles/pmc_lauum.json (separate rocprofv3 --pmc passes of the same kernel; not measured by this run)"
            lauum_kernel = ("gemm_tiles_kernel<true, true, 0, 4, 128, 128>" if args.workload == "c2" else
                            "gemm_tiles_kernel<true, true, 0, 4, 64, 64> (64x64 quadrants: 561 tiles)")
            out["roofline"] = {
                "bound": "mfma", "achieved": achieved, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": achieved / FP64_MFMA_PEAK_TFLOPS, "traffic": traffic, "traffic_from": traffic_from,
                "scope": "whole step: algorithmic flop (T*N^3 + 2N^3/3 + N^2*M = %.4g per GPU) / ms_per_step" % flop_step,
                "kernel": "chol_step_kernel / gemm_tiles_kernel (fp64 MFMA tile engine, every O(N^3) stage); largest "
                          "share of the step: factorisation + inverse (chol_step_kernel launches)",
            }
            if stage_ms:                # --full: the extra step with the stage timers on
                lau_ms, lau_n = stage_ms["lauum"]
                out["roofline"].update({
                    "stages": stage_breakdown(stage_ms, N, 1, M, ms_step, stage_steps),
                    "stages_from": "one extra step after the timed ones, stage timers on (%.1f ms; the timed steps run with "
                                   "the timers off)" % ms_stage_step,
                    "chain_us_per_128": chain_us(stage_ms, N),
                    "dominant_launch": {
                        "kernel": lauum_kernel + " (K^-1 = L^-T L^-1: exactly one launch per Adam iteration, N^3/3 flop)",
                        "launches": lau_n, "avg_launch_ms": lau_ms / max(lau_n, 1),
                        "achieved": (n3 / 3 / (lau_ms / lau_n * 1e-3) / 1e12) if lau_n else None,
                        "traffic": traffic}})
                out["stages_ms_per_call"] = {k: (v[0] / v[1] if v[1] else None) for k, v in stage_ms.items()}
        elif args.workload == "c3cube":
            mean_c, sd_c, hyp = res
            assert mean_c.shape == (M,) and np.isfinite(mean_c).all() and np.isfinite(sd_c).all()
            nblk = 8
            out["config"] = {"workload": ("C3 cube as ONE exact GP: the complete 64x64x64 synthetic hyperspectral cube (N=M=%d), "
                                          "Matern52, %d Adam its (lr 0.1) + posterior on the grid; eight reflection blocks of %d "
                                          "points dealt to the GPUs (gpim_amd/dist_symm.py), all-reduce of 11 doubles per iteration")
                                         % (N, T, N // nblk),
                             "N": N, "M": M, "kernel": "Matern52", "iterations": T, "loss": [float(v) for v in hyp["loss"]],
                             "rms_mean_minus_data": float(np.sqrt(np.mean((mean_c - cube_full.ravel()) ** 2)))}
            nq = float(N // nblk)
            flop_step = nblk * (T * nq ** 3 + 2 * nq ** 3 / 3 + nq * nq * nq)
            achieved = flop_step / (ms_step * 1e-3) / 1e12 / world
            out["roofline"] = {"bound": "mfma", "achieved": achieved, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                               "frac": achieved / FP64_MFMA_PEAK_TFLOPS, "traffic": None,
                               "scope": "whole step per GPU: the blocks' own flop, 8 x (T*Nq^3 + 2Nq^3/3 + Nq^2*Nq), Nq = N/8; the "
                                        "variance's solve runs on the Nq points of the fundamental domain only "
                                        "(the dense model of the same cube: 64x the N^3 terms) / ms_per_step / n_gpus; set-up "
                                        "(workspace allocation, 193 GiB over the ranks) is inside the step"}
        elif args.workload == "c2full":
            mean_f, sd_f, nll_f = res
            assert mean_f.shape == (M,) and np.isfinite(mean_f).all() and np.isfinite(sd_f).all() and np.isfinite(nll_f)
            rms = float(np.sqrt(np.mean((mean_f - yall) ** 2)))
            out["config"] = {"workload": ("C2 complete: 256x256 synthetic twisted-lattice image, ALL pixels observed "
                                          "(N=%d), ONE Matern52 exact GP across the GPUs at fixed hyper-parameters: "
                                          "block-column-cyclic Cholesky + distributed solves + posterior mean and sd on "
                                          "the grid (M=%d)") % (N, M),
                             "N": N, "M": M, "kernel": "Matern52", "hyperparameters": hyper,
                             "rms_mean_minus_data": rms, "nll": nll_f}
            flop_step = float(N) ** 3 / 3.0 + float(N) ** 2 * M
            achieved = flop_step / (ms_step * 1e-3) / 1e12 / world
            out["roofline"] = {"bound": "mfma", "achieved": achieved, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                               "frac": achieved / FP64_MFMA_PEAK_TFLOPS, "traffic": None,
                               "scope": "whole step per GPU: (N^3/3 factorisation + N^2*M variance solves) / ms_per_step / "
                                        "n_gpus; factorisation and variance solves on the MFMA tile engine (gpimhip_dist_*)"}
        else:
            mean_c, sd_c = res
            assert mean_c.shape == cube.shape and np.isfinite(mean_c).all() and np.isfinite(sd_c).all()
            out["config"] = {"workload": ("C3: 64x64x64 synthetic hyperspectral cube, 30%% of the (x,y) columns "
                                          "observed, 64 per-slice 2-D exact GPs (N=%d, M=%d), RBF, T=%d Adam its + "
                                          "predict; slices dealt to the GPUs, concurrent lock-step batches per GPU (batch='auto': four batches of 16 slices on one GPU, four batches of 2 on each of eight)")
                                         % (N, M, T), "N": N, "M": M, "iterations": T, "kernel": "RBF", "slices": 64}
            flop_step = 64 * (T * float(N) ** 3 + 2.0 * float(N) ** 3 / 3.0 + float(N) ** 2 * M)
            achieved = flop_step / (ms_step * 1e-3) / 1e12 / world
            out["roofline"] = {"bound": "mfma", "achieved": achieved, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                               "frac": achieved / FP64_MFMA_PEAK_TFLOPS, "traffic": None,
                               "scope": "whole step per GPU: 64 x (T*N^3 + 2N^3/3 + N^2*M) flop / ms_per_step / n_gpus"}
            if stage_ms:                # --full: the extra step with the stage timers on
                out["roofline"]["scope"] += ("; stages: one extra step with rank 0's slices as ONE lock-step batch of %d "
                                             "problems per launch (share_of_step is relative to the concurrent timed step)"
                                             % nprob)
                out["roofline"].update({"stages": stage_breakdown(stage_ms, N, nprob, M, ms_step, stage_steps),
                                        "stages_from": "one extra step after the timed ones (timers off in the timed steps: "
                                                       "they replay a captured iteration)",
                                        "chain_us_per_128": chain_us(stage_ms, N)})
                out["stages_ms_per_call"] = {k: (v[0] / v[1] if v[1] else None) for k, v in stage_ms.items()}
        if world == 1 and not args.full:
            out["cpu_baseline"] = None
        elif world == 1:
            if args.no_cpu_baseline:
                out["cpu_baseline"] = None
            elif args.workload == "c2":
                out["cpu_baseline"] = cpu_baseline(N, M, T)
                # The timed oracle run IS a full-size reference result: one Adam iteration from the seeded draw and the
                # posterior on all M grid points at N = 16384.  The engine repeats exactly that (same image, same seed).
                orc = out["cpu_baseline"].pop("_oracle_full", None)
                if orc:
                    rec_h = gpim_amd.reconstructor(X, R, Xf, iterations=orc["iterations"], verbose=0, seed=0, **kw)
                    mean_h, sd_h, hyp_h = rec_h.run()
                    rel = lambda a, b: float(np.max(np.abs(np.asarray(a, dtype=float) - np.asarray(b, dtype=float))
                                                    / np.abs(np.asarray(b, dtype=float))))
                    out["rmse_vs_oracle_headline"] = {
                        "config": "the headline workload itself (C2: N=%d, M=%d, Matern52), %d Adam iteration(s) from the "
                                  "seeded draw + predict; oracle = the full-size run timed for cpu_baseline" % (N, M, orc["iterations"]),
                        "rmse_mean": float(np.sqrt(np.mean((mean_h - orc["mean"]) ** 2))),
                        "rmse_sd": float(np.sqrt(np.mean((sd_h - orc["sd"]) ** 2))),
                        "max_abs_mean": float(np.max(np.abs(mean_h - orc["mean"]))),
                        "max_abs_sd": float(np.max(np.abs(sd_h - orc["sd"]))),
                        "hyperparams_max_rel": max(rel(hyp_h["lengthscale"], orc["hyper"]["lengthscale"]),
                                                   rel(hyp_h["noise"], orc["hyper"]["noise"]),
                                                   rel(hyp_h["variance"], orc["hyper"]["variance"]))}
                    del rec_h
            elif args.workload == "c1":
                out["cpu_baseline"] = cpu_baseline_c1(R, T)
            else:
                out["cpu_baseline"] = None
            if not args.no_extra and args.workload == "c2":
                # in a child process: the other configs launch the same kernel instantiations at other sizes,
                # and would blur the per-kernel averages of a `rocprofv3 --stats` run of this command
                import subprocess
                # (bounded: the headline line must not depend on the extras -- they take ~25 s; the concurrent C3 / C5 steps
                # run on several host threads and streams)
                try:
                    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--extras-only"],
                                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
                    out.update(json.loads(child.stdout.strip().splitlines()[-1]))
                except subprocess.TimeoutExpired:
                    out["extra"] = {"error": "extras child did not finish within 600 s"}
                except Exception:
                    out["extra"] = {"error": (child.stderr or child.stdout)[-400:]}
        print(json.dumps(out))
    if world > 1:
        gdist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
