"""Multi-output GP timing on a twin of the reference notebook's EELS run (GP_EELS.ipynb cell 19: 48 x 48 image, 6 NMF
components, N = 2304, T = 6, Matern52, lengthscale bounds [0.5, 2.5], lr 0.05, 200 iterations, prediction on the x2 grid).
Prints one JSON line.  The reference's published 3.05 s/iteration and 603.5 s training (Colab GPU, GPyTorch) are context,
not a same-node comparison."""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "..")); sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import gpim_amd
from test_gpu_vgp import eels_twin

its = int(sys.argv[1]) if len(sys.argv) > 1 else 200
Z = eels_twin()
X, Xd = gpim_amd.utils.get_full_grid(Z[..., 0]), gpim_amd.utils.get_full_grid(Z[..., 0], dense_x=0.5)
runs = []
for rep in range(3):
    rec = gpim_amd.vreconstructor(X, Z, kernel="Matern52", lengthscale=[0.5, 2.5], learning_rate=0.05, iterations=its,
                                  verbose=0)
    torch.cuda.synchronize(); t0 = time.time()
    rec.train(); torch.cuda.synchronize(); t1 = time.time()
    mean, sd = rec.predict(Xd); torch.cuda.synchronize(); t2 = time.time()
    runs.append((t1 - t0, t2 - t1))
train_s, pred_s = min(r[0] for r in runs), min(r[1] for r in runs)
N, T = rec.X.shape[0], rec.num_tasks
flop = T * float(N) ** 3          # per block: factor N^3/3 + triangular inverse N^3/3 + K^-1 = L^-T L^-1 N^3/3
ms_iter = train_s / its * 1e3
print(json.dumps({"problem": "eels_twin_48x48x6", "N": N, "T": T, "iterations": its, "ms_per_iter": round(ms_iter, 3),
                  "train_s": round(train_s, 3), "train_s_200": round(ms_iter * 0.2, 3), "predict_s": round(pred_s, 4),
                  "predict_points": int(np.prod(Xd.shape[1:])), "tflops": round(flop / (ms_iter * 1e-3) / 1e12, 2),
                  "peak_fraction": round(flop / (ms_iter * 1e-3) / 78.6e12, 3),
                  "final_lengthscale": [round(v, 4) for v in rec.hyperparams["lengthscale"][-1]],
                  "context_reference": {"s_per_iter": 3.05, "train_s": 603.5, "where": "Colab GPU, GPyTorch (published)"}}))
