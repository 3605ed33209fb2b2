"""CPU checks of the multi-output GP (no GPU): the block reduction's loss and gradient formulas against the dense
restatement's autograd, the lengthscale parameterisation pinned by the reference notebook, and the public names."""
import inspect

import numpy as np
import pytest

import vgp_oracle as V


@pytest.mark.parametrize("independent", [False, True])
@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("kernel,isotropic,bounds", [("RBF", False, ([0.5, 0.3], [2.5, 4.0])),
                                                      ("Matern52", True, None)])
def test_reduction_equals_dense_autograd(independent, T, kernel, isotropic, bounds):
    X, Y = V.random_data(40, T, 2, seed=T)
    n_ls = 1 if isotropic else 2
    if bounds is not None and isotropic:
        bounds = (bounds[0][0], bounds[1][0])
    u = V.random_u(T, n_ls, independent, seed=10 + T)
    dense = V.Dense(X, Y, kernel, independent, bounds, isotropic)
    l0, g0 = dense.loss_grad(u)
    l1, g1 = V.reduction_loss_grad(u, X, Y, kernel, independent, bounds, isotropic)
    assert abs(l1 - l0) <= 1e-11 * abs(l0)
    assert np.abs(g1 - g0).max() <= 1e-11 * np.abs(g0).max()


@pytest.mark.parametrize("independent", [False, True])
def test_reduction_with_identical_tasks(independent):
    """All tasks equal (the independent model at its initial state: B~ a multiple of I, every lambda_t the same): the
    formulas use no eigenvector derivatives, so the repeated eigenvalues are harmless."""
    T = 4
    X, Y = V.random_data(35, 1, 2, seed=3)
    Y = np.repeat(Y, T, axis=1)
    u = V.initial_u(T, 2, independent=True) if independent else V.initial_u(T, 2, False)
    if not independent:
        u[T:2 * T] = 0.4          # F with equal entries: B = 0.16 11^T + softplus(0) I, two distinct eigenvalues, one repeated
    dense = V.Dense(X, Y, "Matern52", independent, ([0.5, 0.5], [2.5, 2.5]))
    l0, g0 = dense.loss_grad(u)
    l1, g1 = V.reduction_loss_grad(u, X, Y, "Matern52", independent, ([0.5, 0.5], [2.5, 2.5]))
    assert abs(l1 - l0) <= 1e-11 * abs(l0)
    assert np.abs(g1 - g0).max() <= 1e-11 * np.abs(g0).max()


def test_first_adam_step_moves_lengthscale_by_lr():
    """The reference notebook (GP_EELS.ipynb cell 19: bounds [0.5, 2.5], lr 0.05) prints `length: [1.525 1.525]` after
    the first step: the Interval midpoint 1.5 moved by one Adam step of ~lr in raw space (slope (hi - lo) / 4 = 0.5)."""
    X, Y = V.random_data(30, 3, 2, seed=5)
    u0 = V.initial_u(3, 2, False)
    dense = V.Dense(X, Y, "Matern52", False, (0.5, 2.5))
    assert np.allclose(dense.params(u0)[3].numpy(), 1.5)
    hist, _, _ = dense.fit(u0, 0.05, 1)
    step = np.abs(hist[0] - 1.5)          # 2 (sigmoid(0.05) - 1/2) = 0.0249948: Adam's first step is lr in raw space
    assert np.allclose(step, 2.0 * (1.0 / (1.0 + np.exp(-0.05)) - 0.5), rtol=1e-6)
    assert np.all(np.round(step, 3) == 0.025)


def test_alias_module_and_signature():
    import gpim_amd
    from gpim.gpreg.vgpr import vreconstructor
    assert vreconstructor is gpim_amd.vreconstructor
    sig = inspect.signature(vreconstructor.__init__)
    names = list(sig.parameters)
    assert names == ["self", "X", "y", "Xtest", "kernel", "lengthscale", "independent", "learning_rate", "iterations",
                     "use_gpu", "verbose", "seed", "kwargs"]
    defaults = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == {"Xtest": None, "kernel": "RBF", "lengthscale": None, "independent": False, "learning_rate": .1,
                        "iterations": 50, "use_gpu": 1, "verbose": 1, "seed": 0}
    assert list(inspect.signature(vreconstructor.predict).parameters) == ["self", "Xtest", "kwargs"]
    assert list(inspect.signature(vreconstructor.train).parameters) == ["self", "kwargs"]
    assert list(inspect.signature(vreconstructor.run).parameters) == ["self"]


def test_host_parameter_maps_match_oracle():
    """gpim_amd.vgpr.constrained (the trained B, s, mu, l attributes) == the oracle's torch maps."""
    from gpim_amd.vgpr import constrained, raw_layout
    for independent in (False, True):
        T, n_ls = 3, 2
        u = V.random_u(T, n_ls, independent, seed=7)
        assert raw_layout(T, n_ls, independent)[1] == V.layout(T, n_ls, independent)[1] == u.size
        for bounds in (None, (np.array([0.5, 0.2]), np.array([2.5, 3.0]))):
            got = constrained(u, T, n_ls, independent, bounds)
            ref = [t.numpy() for t in V.params_torch(__import__("torch").as_tensor(u), T, n_ls, independent, bounds)]
            for a, b in zip(got, ref):
                assert np.allclose(a, b, rtol=1e-15, atol=0)
