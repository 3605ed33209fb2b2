"""
The mathematics of the spectral-mixture GP's pathwise draws, fixed on the CPU in float64 before any
kernel -- the construction of tests/test_pathwise_host.py with the covariance of sm_oracle.kmat: the recipe of
tests/sm_sample_oracle.py applied to the columns of the identity gives the matrix A with p = A z, and A A^T must be the
posterior covariance of the jittered process,

    Sigma_pw = K_GG + d I - (K_GX + d P)(K + s I)^-1 (K_GX + d P)^T,        s = noise (the model has no jitter).

Bar: both sides are float64 evaluations of the same matrix; the only ill-conditioned step on either side is the solve with
K + s I, so they may differ by a modest multiple of eps * cond(K + s I) * sum w.  TOL takes 100 for that multiple (matrix
orders up to 170 here) -- a number fixed by this reasoning, not by what the code gives; the measured figures are printed and
recorded in sm_sample_oracle.HOST_DISCREPANCY_OVER_SW / COV_SHIFT_OVER_D, which the GPU tests scale.  Leaving the
d scatter(idx, alpha) term out must break the identity by more than TOL where K + s I is well conditioned (random_u).
"""
import functools

import numpy as np
import pytest

import pathwise_oracle as PO
import sm_oracle as SO
import sm_sample_oracle as SSO

# (grid shape, N, Q, isotropic)
GRIDS = (((6, 5), 7, 3, False), ((6, 5), 30, 3, False), ((13, 10), 40, 16, True), ((4, 3, 4), 9, 2, True))
CASES = tuple(g + (gen,) for g in GRIDS for gen in ("random_u", "narrow_u"))
EPS = np.finfo(np.float64).eps


def case_id(c):
    return "%s-N%d-Q%d%s-%s" % ("x".join(str(n) for n in c[0]), c[1], c[2], "-iso" if c[3] else "", c[4])


@functools.lru_cache(maxsize=None)
def make(shape, N, Q, iso, gen, seed=1):
    d = len(shape)
    D = 1 if iso else d
    P = SSO.Params(SSO.GENERATORS[gen](Q, D, seed + 11 * Q), Q, D)
    Xg, _ = PO.full_grid(shape)
    blocks = SSO.Blocks(Xg)
    idx = np.sort(np.random.default_rng(seed).permutation(blocks.M)[:N]).astype(np.int64)
    return P, blocks, idx


def tol(P, blocks, idx):
    X = blocks.G[idx]
    return 100.0 * EPS * PO.cond_spd(P.kmat(X, X) + P.s * np.eye(len(idx))) * P.var


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_covariance_identity(case):
    P, blocks, idx = make(*case)
    A = SSO.probe_matrix(P, blocks, idx)
    Spw = SSO.sigma_pathwise(P, blocks, idx)
    err = np.abs(A @ A.T - Spw).max()
    t = tol(P, blocks, idx)
    A0 = SSO.probe_matrix(P, blocks, idx, scatter=False)
    err0 = np.abs(A0 @ A0.T - Spw).max()
    Sj = SSO.sigma_joint(P, blocks, idx)
    shift = np.abs(Spw - Sj).max() / P.jitter
    print("A A^T - Sigma_pw %.3e (bar %.3e), / sum w %.3e; without the scatter term %.3e; max|Sigma_pw - Sigma| / d %.4f; "
          "noise %.4g, sum w %.4g" % (err, t, err / P.var, err0, shift, P.noise, P.var))
    assert err <= t
    # without the scatter term the covariance is off by d^2 P (K + s I)^-1 P^T: >= d^2 / (sum w + s) on the diagonal
    assert err0 >= 0.5 * P.jitter ** 2 / (P.var + P.s) > 10.0 * err
    # the figures the GPU tests scale (recorded in the oracle module) bound what is measured here
    # (rounding differs between BLAS builds: the recorded discrepancy is held to a factor of two)
    assert err / P.var <= 2.0 * SSO.HOST_DISCREPANCY_OVER_SW
    assert shift <= SSO.COV_SHIFT_OVER_D
    # the closed form of the difference to the joint route's covariance
    X = blocks.G[idx]
    Ai = np.linalg.inv(P.kmat(X, X) + P.s * np.eye(len(idx)))
    Pm = np.zeros((blocks.M, len(idx)))
    Pm[idx, np.arange(len(idx))] = 1.0
    Kgx = P.kmat(blocks.G, X)
    d = P.jitter
    diff = -d * (Pm @ Ai @ Kgx.T + Kgx @ Ai @ Pm.T) - d * d * Pm @ Ai @ Pm.T
    assert np.abs((Spw - Sj) - diff).max() <= t


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_constant_mean_and_blocks_recipe(case):
    """The constant mean enters as y - c and + c: the recipe's mean is sm_oracle.predict's; with an observation on every
    grid point the block recipe gives the pathwise recipe's draws (idx = arange(M)), and the joint recipe's mean and
    variance are sm_oracle.predict's."""
    shape, N, Q, iso, gen = case
    P, blocks, idx = make(*case)
    rng = np.random.default_rng(3)
    M = blocks.M
    X = blocks.G[idx]
    y = P.c + rng.standard_normal(N)
    mean_o, var_o = SO.predict(P.u, X, y, blocks.G, P.Q, P.D)
    R = SSO.draws(P, blocks, idx, y, rng.standard_normal((2, 2 * M + N)), False)
    bar = 100.0 * EPS * PO.cond_spd(P.kmat(X, X) + P.s * np.eye(N)) * (P.var + np.abs(y).max())
    assert np.abs(R["mean"] - mean_o).max() <= bar
    J = SSO.joint_draws(P, X, y, blocks.G, rng.standard_normal((2, M)), False)
    assert np.abs(J["mean"] - mean_o).max() <= bar and np.abs(J["var"] - var_o).max() <= bar
    L = SSO.joint_factor(P, X, blocks.G, False)
    assert L.shape == (N + M, N + M) and np.abs(L @ L.T - SSO.joint_matrix(P, X, blocks.G, False, P.jitter)).max() <= 64 * (N + M) * EPS * P.var
    # fully observed: blocks == pathwise with idx = arange(M)
    yg = P.c + rng.standard_normal(M)
    Z = rng.standard_normal((2, 3 * M))
    full = np.arange(M)
    Rp = SSO.draws(P, blocks, full, yg, Z, False)
    Rb = SSO.blocks_draws(P, blocks, yg, Z, False)
    cond = max(Rb["cond"], SSO.condition(P, blocks, full))
    barb = 100.0 * EPS * cond * (P.var + np.abs(yg).max())
    print("blocks vs pathwise: mean %.3e draws %.3e (bar %.3e, cond %.3e)"
          % (np.abs(Rb["mean"] - Rp["mean"]).max(), np.abs(Rb["out"] - Rp["out"]).max(), barb, cond))
    assert np.abs(Rb["mean"] - Rp["mean"]).max() <= barb and np.abs(Rb["out"] - Rp["out"]).max() <= barb


def test_prior_draw_covariance():
    """g = U^T blockdiag(chol(K_b + d I)) z has covariance K_GG + d I for this covariance too (mirror-plane weights: a 5-
    and a 13-point axis)."""
    for case in (CASES[1], CASES[5]):
        P, blocks, _ = make(*case)
        Gm = blocks.prior_draw(P, P.jitter, np.eye(blocks.M)).T
        K = P.kmat(blocks.G, blocks.G) + P.jitter * np.eye(blocks.M)
        assert np.abs(Gm @ Gm.T - K).max() <= 64 * blocks.M * EPS * P.var


def test_narrow_u_is_narrow():
    """narrow_u: noise 1e-4 + softplus(-4) = 0.018; its K + s I is far worse conditioned than random_u's (which stays below
    5 on these cases), which is what exposes a conditioning-dependent error."""
    P, blocks, idx = make((6, 5), 30, 3, False, "narrow_u")
    assert abs(P.noise - (1e-4 + np.log1p(np.exp(-4.0)))) < 1e-15 and abs(P.noise - 0.018) < 5e-4
    X = blocks.G[idx]
    cn = PO.cond_spd(P.kmat(X, X) + P.s * np.eye(len(idx)))
    Pr, _, _ = make((6, 5), 30, 3, False, "random_u")
    cr = PO.cond_spd(Pr.kmat(X, X) + Pr.s * np.eye(len(idx)))
    print("cond(K + s I): narrow_u %.3e, random_u %.3e" % (cn, cr))
    assert cn > 20.0 * cr


def test_oracle_rejects_bad_jitter():
    P, blocks, idx = make((6, 5), 7, 3, False, "random_u")
    for d in (0.0, -1e-6, P.s * 1.01):
        with pytest.raises(ValueError):
            SSO.draws(P, blocks, idx, np.zeros(len(idx)), np.zeros((1, blocks.M + len(idx))), True, d=d)
    with pytest.raises(ValueError):
        SSO.joint_draws(P, blocks.G[idx], np.zeros(len(idx)), blocks.G, np.zeros((1, blocks.M)), True, d=-1e-9)


def test_binding_has_the_entries(ensure_built):
    import ctypes
    from gpim_amd import _lib
    lib = _lib.load()
    for name, nargs in (("gpimhip_sample_sm", 15), ("gpimhip_sample_sm_pathwise", 16), ("gpimhip_sample_sm_blocks", 14)):
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs
    # no handle: refused before anything touches a device
    assert lib.gpimhip_sample_sm(None, None, None, None, 1, None, None, 1, None, 1, 0, 1e-5, None, None, None) == _lib.E_BADARG
    assert lib.gpimhip_sample_sm_pathwise(None, None, None, None, 1, None, None, None, 1, None, None, 1, 0, 1e-5, None,
                                          None) == _lib.E_BADARG
    assert lib.gpimhip_sample_sm_blocks(None, None, None, None, 1, None, None, None, None, 1, 0, 1e-5, None, None) == _lib.E_BADARG


def test_python_surface_names():
    import inspect
    import gpim_amd
    from gpim_amd import _sampling, smgpr
    sig = inspect.signature(smgpr.smreconstructor.sample)
    assert list(sig.parameters)[1:] == ["n_samples", "Xtest", "noiseless", "seed", "z", "jitter", "method"]
    assert sig.parameters["method"].default == "joint" and sig.parameters["jitter"].default is None
    assert set(_sampling.SPECTRAL_METHODS) == {"joint", "pathwise", "blocks"}
    # one host path: the spectral methods are the dense ones with their gate, jitter source and call replaced
    for name, m in _sampling.SPECTRAL_METHODS.items():
        assert isinstance(m, type(_sampling.METHODS[name])) and type(m).plan is not None
