"""
The two CPU references of the structured (Kronecker) exact GP against each other, no GPU: the dense oracle
(oracle/gpim_oracle.py: ExactGP -- Cholesky of the N x N matrix, autograd) and the numpy eigenbasis evaluation of
tests/kron_oracle.py.

  * small grids (every layout of tests/test_gpu_kron.py: ARD, isotropic, 3D, 4D, an axis of one point): the two agree to the
    bars the device is held to there, so the second reference states the same model;
  * the large cases (kron_oracle.BIG_CASES): the two are still within 2 x the distances recorded in kron_oracle.DISTANCES,
    from which tests/test_gpu_kron.py derives the device's bars.  A drift of either reference shows here, on the CPU.
"""
import numpy as np
import pytest
import torch

import kron_oracle as KO
from oracle import gpim_oracle as O


@pytest.mark.parametrize("shape,iso", [((12, 10), False), ((9, 14), True), ((6, 5, 8), False), ((4, 3, 5, 4), False),
                                       ((1, 7), False)])
def test_references_agree_on_small_grids(shape, iso):
    d = len(shape)
    R = KO.smooth_grid(shape, seed=sum(shape))
    axes = [np.arange(n, dtype=np.float64) for n in shape]
    ls = [0.7, 9.0] if iso else [[0.7] * d, [9.0] * d]
    torch.manual_seed(2)
    kp = O.KernelParams("RBF", d, ls)
    with torch.no_grad():
        kp.u_noise.fill_(-2.5)
    X = torch.from_numpy(np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, d))
    gp = O.ExactGP(X, torch.from_numpy(R.ravel()), kp, KO.JITTER)
    loss_ref, g_ref = gp.loss_and_grad()
    u = np.concatenate([[kp.u_var.item()], kp.u_ls.detach().numpy().reshape(-1), [-2.5]])
    kg = KO.KronGP(axes, R, u, ls[0], ls[1])
    loss, g = kg.loss_and_grad()
    assert abs(loss - loss_ref.item()) <= KO.LOSS_RTOL * abs(loss_ref.item())
    g_ref = g_ref.numpy()
    assert np.all(np.abs(g - g_ref) <= KO.GRAD_RTOL * np.abs(g_ref) + KO.GRAD_ATOL * max(1.0, np.abs(g_ref).max()))
    taxes = [np.linspace(-0.5, n - 0.5, 2 * n + 1) for n in shape]
    Xs = torch.from_numpy(np.stack(np.meshgrid(*taxes, indexing="ij"), -1).reshape(-1, d))
    mref, vref = gp.predict(Xs)
    mean, var = kg.predict(taxes)
    assert np.abs(mean - mref.numpy()).max() <= KO.POST_ATOL
    assert np.abs(var - vref.numpy()).max() <= KO.POST_ATOL


@pytest.mark.parametrize("shape,u_noise", KO.BIG_CASES, ids=lambda v: str(v))
def test_references_stay_within_recorded_distances(shape, u_noise):
    now, rec = KO.distances(shape, u_noise), KO.DISTANCES[(shape, u_noise)]
    print("%s u_noise %g: measured %r\n    recorded %r" % (shape, u_noise, now, rec))
    assert now["loss_rel"] <= 2 * rec["loss_rel"]
    assert np.all(np.asarray(now["grad_abs"]) <= 2 * np.asarray(rec["grad_abs"]))
    assert now["mean_abs"] <= 2 * rec["mean_abs"]
    assert now["var_abs"] <= 2 * rec["var_abs"]


def test_device_bars_never_go_below_the_small_size_bars():
    for (shape, un), rec in KO.DISTANCES.items():
        g = np.array([10.0, -300.0, 50.0, 200.0])
        la, ga, ma, va = KO.device_bars(shape, un, 500.0, g)
        assert la >= KO.LOSS_RTOL * 500.0 and la >= 10 * rec["loss_rel"] * 500.0
        assert np.all(ga >= KO.GRAD_RTOL * np.abs(g) + KO.GRAD_ATOL * 300.0) and np.all(ga >= 10 * np.asarray(rec["grad_abs"]))
        assert ma >= KO.POST_ATOL and va >= KO.POST_ATOL and ma >= 10 * rec["mean_abs"] and va >= 10 * rec["var_abs"]
