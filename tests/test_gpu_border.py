"""skreconstructor on incomplete grids: the reflection blocks of the completed grid with a border for the missing points
(csrc/border.hip) against the dense exact GP on the observed points."""
import time

import numpy as np
import pytest
import torch

import gpim_amd
from problems import gpr_dummy_data, spiral_image

pytestmark = pytest.mark.gpu


def _image(n, frac, seed=0, shape=None):
    shape = shape or (n, n)
    rng = np.random.default_rng(seed)
    grids = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")
    R = np.cos(grids[0] / 5.0) * np.sin(grids[1] / 7.0 + 0.3)
    for k in range(2, len(shape)):
        R = R + 0.3 * np.cos(grids[k] / 3.0)
    R = R + 0.05 * rng.standard_normal(shape)
    flat = rng.choice(R.size, size=max(1, int(round(frac * R.size))), replace=False)
    R.ravel()[flat] = np.nan
    return R


def _pair(R, kernel, force=False, **kw):
    X = gpim_amd.utils.get_sparse_grid(R)
    Xf = gpim_amd.utils.get_full_grid(R)
    kw = dict(dict(learning_rate=0.1, iterations=1, verbose=0), **kw)
    if force:
        # the border engine whatever the solver choice would be (large fractions missing)
        b = gpim_amd.reconstructor(X, R, Xf, kernel=kernel, structured=True, _border=gpim_amd.utils.border_blocks(X, R), **kw)
        b.solver = "border"
    else:
        b = gpim_amd.skreconstructor(X, R, Xf, kernel=kernel, **kw)
    d = gpim_amd.reconstructor(X, R, Xf, kernel=kernel, **kw)
    return b, d, Xf


@pytest.mark.parametrize("kernel", ["RBF", "Matern52"])
def test_reference_skgpr_2d(kernel):
    # the reference's test_skgpr_2d: 20 x 20 with up to 200 NaN, 2 iterations
    R = gpr_dummy_data()
    X, Xf = gpim_amd.utils.get_sparse_grid(R), gpim_amd.utils.get_full_grid(R)
    rec = gpim_amd.skreconstructor(X, R, Xf, kernel=kernel, learning_rate=0.1, iterations=2, verbose=0)
    assert rec.solver in ("border", "dense")
    mean, sd, _ = rec.run()
    assert mean.shape == R.shape and sd.shape == R.shape
    assert np.isfinite(mean).all() and np.isfinite(sd).all()


PARITY = [
    ("RBF", (32, 32), 1),
    ("Matern52", (32, 32), 0.05),
    ("RationalQuadratic", (31, 32), 0.1),
    ("Matern52", (33, 33), 0.3),
    ("RBF", (16, 16, 15), 0.05),
    ("Matern52", (64, 64), 0.1),
]


@pytest.mark.parametrize("kernel,shape,frac", PARITY)
def test_loss_grad_parity(kernel, shape, frac):
    R = _image(None, frac if frac < 1 else 1.0 / np.prod(shape), seed=2, shape=shape)
    for iso in (False, True):
        b, d, _ = _pair(R, kernel, force=frac >= 0.2, isotropic=iso) if iso else _pair(R, kernel, force=frac >= 0.2)
        assert b.solver == "border", (shape, frac)
        d._u.copy_(b._u)
        lb, gb = b.loss_and_grad()
        ld, gd = d.loss_and_grad()
        assert abs(lb - ld) <= 1e-9 * abs(ld), (lb, ld)
        rel = ((gb - gd).abs() / gd.abs().clamp(min=1e-300)).max().item()
        assert rel <= 1e-9, (gb, gd)


def test_training_and_prediction_match_dense():
    R = _image(64, 0.05, seed=3)
    b, d, Xf = _pair(R, "Matern52", iterations=30)
    assert b.solver == "border"
    mb, sb, hb = b.run()
    md, sd, hd = d.run()
    for key in ("lengthscale", "noise", "variance"):
        assert np.allclose(np.asarray(hb[key]), np.asarray(hd[key]), rtol=1e-6, atol=0), key
    assert np.allclose(b.loss_all, d.loss_all, rtol=1e-6, atol=0)
    print("max |mean| dev %.2e, max |sd| dev %.2e" % (np.abs(mb - md).max(), np.abs(sb - sd).max()))
    assert np.abs(mb - md).max() < 1e-7 and np.abs(sb - sd).max() < 1e-7
    Xh = gpim_amd.utils.get_full_grid(R, dense_x=0.5)
    mb2, sb2 = b.predict(Xh)
    md2, sd2 = d.predict(Xh)
    print("dense_x=0.5: max |mean| dev %.2e, max |sd| dev %.2e" % (np.abs(mb2 - md2).max(), np.abs(sb2 - sd2).max()))
    assert np.abs(mb2 - md2).max() < 1e-7 and np.abs(sb2 - sd2).max() < 1e-7


def test_solver_choice():
    Rs, _ = spiral_image(size=128)
    X = gpim_amd.utils.get_sparse_grid(Rs)
    assert gpim_amd.skreconstructor(X, Rs, None, kernel="Matern52", verbose=0).solver == "dense"
    R = _image(128, 0.05, seed=4)
    rec = gpim_amd.skreconstructor(gpim_amd.utils.get_sparse_grid(R), R, None, kernel="Matern52", verbose=0)
    assert rec.solver == "border"
    with pytest.raises(NotImplementedError):
        rec.model.y = rec.model.y
    # reconstructor(structured=True) keeps refusing NaN
    with pytest.raises(NotImplementedError):
        gpim_amd.reconstructor(gpim_amd.utils.get_sparse_grid(R), R, None, kernel="Matern52", structured=True, verbose=0)


def test_border_bitwise_repeatable():
    R = _image(48, 0.1, seed=5)
    outs = []
    for _ in range(2):
        b, _, _ = _pair(R, "RationalQuadratic", iterations=12)
        m, s, h = b.run()
        outs.append((m, s, np.asarray(b.loss_all)))
    for a, c in zip(outs[0], outs[1]):
        assert np.array_equal(a, c)


def test_large_image_two_percent():
    R = _image(256, 0.02, seed=6)
    X, Xf = gpim_amd.utils.get_sparse_grid(R), gpim_amd.utils.get_full_grid(R)
    rec = gpim_amd.skreconstructor(X, R, Xf, kernel="Matern52", learning_rate=0.1, iterations=1, verbose=0)
    assert rec.solver == "border"
    rec.train(iterations=1)
    torch.cuda.synchronize()
    t0 = time.time()
    rec.train(iterations=4)
    torch.cuda.synchronize()
    dt = (time.time() - t0) / 4
    print("256x256, 2%% missing: %.3f s per Adam iteration" % dt)
    assert rec.loss_all[-1] < rec.loss_all[0]
    mean, sd = rec.predict()
    assert np.isfinite(mean).all() and np.isfinite(sd).all()
    miss = np.isnan(R)
    noise_sd = np.sqrt(rec.noise_all[-1])
    assert np.median(sd[~miss]) < 1.5 * noise_sd
    # the latent variance (sd^2 - noise) away from the image edges: larger where the pixel is missing
    latent = sd ** 2 - rec.noise_all[-1]
    inner = np.zeros_like(miss)
    inner[8:-8, 8:-8] = True
    assert np.median(latent[miss & inner]) > np.median(latent[~miss & inner])
