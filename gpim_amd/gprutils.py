"""
gprutils.py -- grid and data-layout helpers of the hot path (exported as ``gpim_amd.utils``).

Host-side mirror of the data-prep part of the reference's gpim/gprutils.py:23-210
(SURVEY 8(a) rows a1-a3): ``(c, *dims)`` coordinate grids <-> ``(N, c)`` row-major point
lists, NaN filtering, full / sparse index grids.  Plotting and corruption helpers of the
reference file (:213-938) are outside the hot path and not provided.
"""
import ctypes

import numpy as np
import torch


def _np_dtype(precision):
    return np.float32 if precision == "single" else np.float64


def prepare_training_data(X, y=None, vector_valued=False, **kwargs):
    """(c,*dims) grid + (*dims) observations -> torch tensors X:(N,c), y:(N,).

    Rows of X with any NaN coordinate are dropped and NaN entries of y are dropped; the
    two NaN patterns are expected to coincide (true for grids from ``get_sparse_grid``).
    Row-major order is preserved (reference gprutils.py:23-59).
    """
    dt = _np_dtype(kwargs.get("precision", "double"))
    pts = np.asarray(X).reshape(X.shape[0], -1).T
    pts = pts[~np.isnan(pts).any(axis=1)]
    Xt = torch.from_numpy(np.ascontiguousarray(pts, dtype=dt))
    if y is None:
        return Xt, y
    if vector_valued:
        yv = np.asarray(y).reshape(-1, y.shape[-1])
        yv = yv[~np.isnan(yv).any(axis=1)]
    else:
        yv = np.asarray(y).ravel()
        yv = yv[~np.isnan(yv)]
    return Xt, torch.from_numpy(np.ascontiguousarray(yv, dtype=dt))


def prepare_test_data(X, **kwargs):
    """(c,*dims) -> (M,c) torch tensor; NaN rows are kept (reference gprutils.py:62-85)."""
    dt = _np_dtype(kwargs.get("precision", "double"))
    pts = np.asarray(X).reshape(X.shape[0], -1).T
    return torch.from_numpy(np.ascontiguousarray(pts, dtype=dt))


def get_full_grid(R, extent=None, dense_x=1.):
    """Index coordinates of a 2D-4D array as an array of shape (ndim, *grid)
    (reference gprutils.py:108-172).  ``dense_x`` < 1 refines the grid; ``extent``
    ([[lo, hi], ...] per dimension) places it in physical units.  The reference only
    works with ``extent`` in 2D (its 3D/4D branches fail to unpack); here every
    dimensionality follows the 2D rule."""
    nd = np.ndim(R)
    if nd < 2 or nd > 4:
        raise NotImplementedError("Currently works only for 2D-4D sets")
    dense_x = np.float64(dense_x)
    if extent:
        axes = []
        for n, (lo, hi) in zip(np.shape(R), extent):
            axes.append(slice(lo, hi, dense_x / (n // (hi - lo))))
    else:
        axes = [slice(None, n, dense_x) for n in np.shape(R)]
    return np.array(np.mgrid[tuple(axes)])


def get_sparse_grid(R, extent=None):
    """Full grid with NaN coordinates at the missing observations of R
    (reference gprutils.py:175-210; 2D, and 3D with xy- or xyz-sparsity)."""
    if not np.isnan(R).any():
        raise NotImplementedError(
            "Missing values in sparse data must be represented as NaNs")
    nd = np.ndim(R)
    if nd not in (2, 3):
        raise NotImplementedError(
            "Currently supports only 2D and 3D sets with sparsity in xy and xyz dims")
    grid = get_full_grid(R, extent)
    missing = np.isnan(R)
    if nd == 3 and not missing[..., -1].any():
        # xy-sparsity: a NaN anywhere in a spectrum removes the whole (x, y) column
        missing = np.broadcast_to(missing.any(axis=-1, keepdims=True), R.shape)
    X = grid.copy()
    X[:, missing] = np.nan
    return X


def get_grid_indices(R, dense_x=1.):
    """(X_full, X_sparse) for a 2D/3D array (reference gprutils.py:88-105)."""
    if np.ndim(R) > 3:
        raise NotImplementedError("Currently supports only 2D and 3D arrays")
    return get_full_grid(R, dense_x=np.float64(dense_x)), get_sparse_grid(R)


def default_lengthscale(shape, isotropic=False):
    """The lengthscale bounds used when none are given: [0, mean(shape) / 2], per dimension or one shared (isotropic)."""
    lmean = float(np.mean(shape) / 2)
    return [0., lmean] if isotropic else [[0.] * len(shape), [lmean] * len(shape)]


def n_inducing(n, indpoints=None):
    """The number of inducing inputs asked of n observations (reference gpr.py:145-153): n // 10 by default, at least 1 and
    at most n; the inducing inputs themselves are X[::n // n_inducing(n, indpoints)]."""
    return max(n // 10, 1) if indpoints is None else min(indpoints, n)


def grid_axes(X):
    """Coordinate vectors of a product grid X (d, n_1, ..., n_d): X[i] must vary along axis i only (what get_full_grid
    returns, with or without ``extent`` / ``dense_x``).  Returns (axes, their lengths as a C int32 array)."""
    X = np.asarray(X, dtype=np.float64)
    d = X.shape[0]
    if X.ndim != d + 1:
        raise NotImplementedError("structured=True needs grid coordinates of shape (d, n_1, ..., n_d)")
    axes = []
    for i in range(d):
        c = np.moveaxis(X[i], i, 0).reshape(X.shape[1 + i], -1)[:, 0].copy()
        shape = [1] * d
        shape[i] = -1
        if not np.array_equal(X[i], np.broadcast_to(c.reshape(shape), X.shape[1:])):
            raise NotImplementedError("structured=True needs a product grid (coordinate i varying along axis i only)")
        axes.append(c)
    return axes, (ctypes.c_int32 * d)(*[len(c) for c in axes])


def union_axes(axes_train, axes_test):
    """Per grid axis, the sorted union of the training and the test coordinates with the position of every coordinate in
    it (gpim_amd extension: reconstructor.sample(method='kron')).

    axes_train, axes_test: d coordinate vectors each.  Coordinates within ``1e-12 * max(1, max|coordinate|)`` of their
    neighbour in sorted order merge (the tolerance of the structured solver's symmetry test); a merged coordinate is
    represented by a training coordinate when it holds one, so axes that bring nothing new leave the training axis as it
    is.  Returns (axes_union, idx_train, idx_test): d float64 vectors and two lists of d int32 index vectors with
    ``axes_union[i][idx_train[i]] ~ axes_train[i]`` and ``axes_union[i][idx_test[i]] ~ axes_test[i]``."""
    if len(axes_train) != len(axes_test):
        raise ValueError("union_axes needs as many test axes as training axes; got %d and %d"
                         % (len(axes_train), len(axes_test)))
    au, ic, it = [], [], []
    for c, t in zip(axes_train, axes_test):
        c = np.asarray(c, dtype=np.float64).ravel()
        t = np.asarray(t, dtype=np.float64).ravel()
        both = np.concatenate([c, t])
        if not np.isfinite(both).all():
            raise ValueError("union_axes needs finite coordinates")
        tol = 1e-12 * max(1.0, float(np.abs(both).max()))
        order = np.argsort(both, kind="stable")
        sv = both[order]
        first = np.concatenate([[True], np.diff(sv) > tol])
        group = np.cumsum(first) - 1
        u = sv[first].copy()
        from_train = order < len(c)
        u[group[from_train][::-1]] = sv[from_train][::-1]       # the first training coordinate of a group stands for it
        idx = np.empty(len(both), dtype=np.int32)
        idx[order] = group
        au.append(u)
        ic.append(idx[:len(c)].copy())
        it.append(idx[len(c):].copy())
    return au, ic, it


def union_rows(Xs, Xt):
    """The sorted (lexicographic) union P of the ragged training rows Xs (N_s, p) and the ragged test rows Xt (M_s, p) with
    the position of every row in it (gpim_amd extension: reconstructor.sample(method='columns')).

    Two rows merge when every coordinate agrees within ``1e-12 * max(1, max|coordinate|)`` (per coordinate column: the
    tolerance of ``union_axes``, applied to neighbours in sorted order); a merged row is represented by the training one when
    it holds one.  Returns (P (U_s, p) float64, i_train (N_s,) int32, i_test (M_s,) int32) with ``P[i_train] ~ Xs`` and
    ``P[i_test] ~ Xt``."""
    Xs = np.asarray(Xs, dtype=np.float64)
    Xt = np.asarray(Xt, dtype=np.float64)
    if Xs.ndim != 2 or Xt.ndim != 2 or Xs.shape[1] != Xt.shape[1]:
        raise ValueError("union_rows needs training rows (N_s, p) and test rows (M_s, p); got %s and %s"
                         % (Xs.shape, Xt.shape))
    both = np.concatenate([Xs, Xt])
    if not np.isfinite(both).all():
        raise ValueError("union_rows needs finite coordinates")
    ids = np.empty(both.shape, dtype=np.int64)
    for k in range(both.shape[1]):
        tol = 1e-12 * max(1.0, float(np.abs(both[:, k]).max()))
        order = np.argsort(both[:, k], kind="stable")
        ids[order, k] = np.cumsum(np.concatenate([[True], np.diff(both[order, k]) > tol])) - 1
    # rows of equal ids are one row; np.unique sorts them lexicographically (ids grow with the coordinate) and names the
    # first row of every group in `both`, a training row whenever the group holds one
    _, first, inv = np.unique(ids, axis=0, return_index=True, return_inverse=True)
    inv = np.asarray(inv).reshape(-1).astype(np.int32)
    return both[first].copy(), inv[:len(Xs)].copy(), inv[len(Xs):].copy()


def column_sample_maps(C, tshape):
    """Index vectors between the caller's layouts and the library's for draws of a ``column_blocks`` model C on a test grid
    of shape tshape: (e_idx, n_idx, o_idx) with ``z_e_lib = z_e[:, e_idx]`` (the training points'
    row order -> (N_s, J)), ``z_n_lib = z_n[:, n_idx]`` (the test grid's C order -> (M_s, M_c), ragged axes first) and
    ``out = out_lib[:, o_idx]`` (back).  All three go through ``C["perm"]``."""
    Ns, J = C["Y"].shape
    rshape = [C["shape"][i] for i in C["ragged"]]
    T = np.full((int(np.prod(rshape)), J), -1, dtype=np.int64)
    T[C["obs"]] = np.arange(Ns * J).reshape(Ns, J)
    T = T.reshape([C["shape"][i] for i in C["perm"]]).transpose(C["inv"]).ravel()
    T = T[T >= 0]                                        # training row t (grid order, NaN dropped) sits at T[t] of (N_s, J)
    M = int(np.prod(tshape, dtype=np.int64))
    n_idx = np.arange(M).reshape(tshape).transpose(C["perm"]).ravel()
    o_idx = np.arange(M).reshape([tshape[i] for i in C["perm"]]).transpose(C["inv"]).ravel()
    return np.argsort(T), n_idx, o_idx


def reflection_blocks(X, y, axes):
    """Symmetry reduction of an exact GP on a COMPLETE grid (gpim_amd extension; role of the reference's structured class
    gpim/gpreg/skgpr.py:399-448 for kernels that do not factorise over the axes -- csrc/engine.hip: kmat_refl_kernel).

    X (d, n_1, ..., n_d) grid coordinates, y (n_1, ..., n_d) observations, axes: the d coordinate vectors.  Every axis whose
    coordinates are symmetric about their centre is reflected; with r such axes the covariance of a stationary kernel that is
    even in each coordinate difference is block diagonal in the basis
        v_{s,p} = (|G| |Stab_p|)^-1/2 sum_g chi_s(g) e_{g p}      (p in the fundamental domain, s one of 2^r sign patterns)
    with blocks  K_s[p, q] = w_p w_q sum_g chi_s(g) k(p, g q),  w_p = |Stab_p|^-1/2.
    Returns a dict: mask (bit k = axis k reflected), twoc (first + last coordinate per axis), B = 2^r, Xq (the fundamental
    domain, (Nq, d): the first half of every reflected axis, including the mirror plane of an axis of odd length), ys (B, Nq):
    y in the adapted basis, wts (B, Nq) or None when no point lies on a mirror plane: w_p, and 0 where the point does not
    exist in the block (it lies on the mirror plane of an axis whose sign is -1), n_total = y.size.
    Raises ValueError if no axis is symmetric."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    d = X.shape[0]
    mask, twoc, dims = 0, [0.0] * 4, []
    for k, c in enumerate(axes):
        c = np.asarray(c, dtype=np.float64)
        if len(c) >= 2 and np.allclose(c + c[::-1], c[0] + c[-1], rtol=0, atol=1e-12 * max(1.0, abs(c[-1]), abs(c[0]))):
            mask |= 1 << k
            twoc[k] = float(c[0] + c[-1])
            dims.append(k)
    if not dims:
        raise ValueError("needs at least one grid axis with coordinates that are symmetric about their centre")
    B = 1 << len(dims)
    fund = tuple(slice(0, (y.shape[k] + 1) // 2) if k in dims else slice(None) for k in range(d))
    Xq = X[(slice(None),) + fund].reshape(d, -1).T.copy()
    fshape = y[fund].shape
    idx = np.indices(fshape)
    # on_plane[j]: the points of the domain on the mirror plane of the j-th reflected axis (odd length only)
    on_plane = [(idx[k] == y.shape[k] // 2) & (y.shape[k] % 2 == 1) for k in dims]
    nplanes = np.sum(on_plane, axis=0)
    w_pt = 2.0 ** (-0.5 * nplanes)                      # 1 / sqrt(|stabiliser|)
    ys, wts = np.empty((B, Xq.shape[0])), np.empty((B, Xq.shape[0]))
    for b in range(B):
        acc = np.zeros(fshape)
        for g in range(B):
            ax = tuple(dims[j] for j in range(len(dims)) if (g >> j) & 1)
            chi = -1.0 if bin(g & b).count("1") & 1 else 1.0
            acc += chi * (np.flip(y, axis=ax) if ax else y)[fund]
        present = np.ones(fshape, dtype=bool)
        for j in range(len(dims)):
            if (b >> j) & 1:
                present &= ~on_plane[j]                 # antisymmetric along an axis: nothing on its mirror plane
        wb = np.where(present, w_pt, 0.0)
        ys[b] = (acc * wb).reshape(-1) / np.sqrt(B)
        wts[b] = wb.reshape(-1)
    # for predictions on the training grid: the domain's points as flat grid indices, and every grid point's representative
    # in the domain (the posterior variance is invariant under the reflections)
    full = np.indices(y.shape)
    fund_flat = np.ravel_multi_index(tuple(full[k][fund] for k in range(d)), y.shape).reshape(-1)
    rep_idx = tuple(np.minimum(full[k], y.shape[k] - 1 - full[k]) if k in dims else full[k] for k in range(d))
    rep = np.ravel_multi_index(rep_idx, fshape).reshape(-1)
    # the reflections that take a grid point's representative to it: bit j = the j-th reflected axis (the numbering of the
    # sign patterns b above); a point on that axis' mirror plane has 0 (leave-one-out combines the blocks with chi_b(sgn))
    sgn = np.zeros(y.shape, dtype=np.int64)
    for j, k in enumerate(dims):
        sgn |= (full[k] > y.shape[k] - 1 - full[k]).astype(np.int64) << j
    return {"mask": mask, "twoc": twoc, "B": B, "Xq": Xq, "ys": ys, "wts": wts if nplanes.any() else None,
            "n_total": int(y.size), "dims": dims, "fund_flat": fund_flat, "rep": rep, "sgn": sgn.reshape(-1)}


def reflection_blocks_multi(X, Y, axes):
    """The reflection blocks of a multi-output GP on a COMPLETE grid (gpim_amd extension: vreconstructor's 'reflection'
    solver).  X (d, n_1, ..., n_d), Y (n_1, ..., n_d, T), axes as for ``reflection_blocks``.

    Returns the dict of ``reflection_blocks`` with ys of shape (T, B, Nq) -- task a in the adapted basis, task-major then
    sign pattern -- and ones (B, Nq) = U 1, the basis change of the constant (sqrt(B) w_0 in block 0, 0 in the others; the
    task means enter the blocks through it).  Raises ValueError if no axis is symmetric."""
    Y = np.asarray(Y, dtype=np.float64)
    T = Y.shape[-1]
    S = reflection_blocks(X, np.ones(Y.shape[:-1]), axes)
    ones = S["ys"]
    S["ys"] = np.stack([reflection_blocks(X, Y[..., a], axes)["ys"] for a in range(T)]) if T else np.empty((0,) + ones.shape)
    S["ones"] = ones
    return S


def complete_grid(X, y):
    """The complete product grid behind an incomplete one (gpim_amd extension: the border form of the reflection blocks,
    reconstructor's exact GP on the observed points of an image or cube with missing pixels).

    X (d, n_1, ..., n_d): grid coordinates with NaN at the missing points (what ``get_sparse_grid`` returns), y
    (n_1, ..., n_d) with NaN at the same points.  Returns (axes, miss): the d coordinate vectors of the completed grid and
    the flat (row-major) indices of the missing points.  Raises NotImplementedError when the observed coordinates do not
    form a product grid, when some index along an axis has no observation, or when the NaN patterns of X and y differ."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    d = X.shape[0]
    if X.ndim != d + 1 or X.shape[1:] != y.shape:
        raise NotImplementedError("grid completion needs coordinates of shape (d, n_1, ..., n_d) and y of shape (n_1, ..., n_d)")
    missing = np.isnan(X).any(axis=0)
    if not np.array_equal(missing, np.isnan(y)):
        raise NotImplementedError("grid completion needs the same NaN pattern in X and y")
    axes = []
    for i in range(d):
        vals = np.moveaxis(X[i], i, 0).reshape(X.shape[1 + i], -1)
        obs = np.moveaxis(~missing, i, 0).reshape(X.shape[1 + i], -1)
        if not obs.any(axis=1).all():
            raise NotImplementedError("grid completion: an index along axis %d has no observation" % i)
        first = np.argmax(obs, axis=1)
        c = vals[np.arange(vals.shape[0]), first]
        if not np.all((vals == c[:, None]) | ~obs):
            raise NotImplementedError("grid completion needs a product grid (coordinate %d varying along axis %d only)" % (i, i))
        axes.append(c)
    return axes, np.flatnonzero(missing.ravel())


def border_blocks(X, y):
    """Reflection blocks of the completed grid plus the "border" of its missing points (gpim_amd extension; DESIGN.md
    section 11).  The exact GP on the observed points is computed from the 2^r blocks B_b of A = K + (noise + jitter) I on
    the completed grid and the M x M matrix S = (A^-1)_mm: A_oo^-1 embedded in the grid is A^-1 - A^-1 P_m S^-1 P_m^T A^-1.

    Returns the dict of ``reflection_blocks`` for the completed grid with y = 0 at the missing points, and in addition: axes,
    miss (flat indices of the M missing points), q (int32, M): each missing point's representative in the fundamental
    domain (a row of Xq), coef (B, M): its coefficient in block b, (U^T e_j)_{b, q(j)} = chi_b(g_j) sqrt(|Stab_q|) / sqrt(B)
    (0 where the point does not exist in the block), n_obs = the number of observations.
    Raises NotImplementedError when the grid cannot be completed, ValueError when no axis is symmetric."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    axes, miss = complete_grid(X, y)
    Xc = np.array(np.meshgrid(*axes, indexing="ij"))
    S = reflection_blocks(Xc, np.nan_to_num(y, nan=0.0), axes)
    dims, B = S["dims"], S["B"]
    idx = np.unravel_index(miss, y.shape)
    q = S["rep"][miss].astype(np.int32)
    # g_j: the reflections that take the representative to the point (bit j = the j-th reflected axis);
    # stab: 2^(mirror planes the representative lies on)
    gbits = np.zeros(len(miss), dtype=np.int64)
    nplanes = np.zeros(len(miss), dtype=np.int64)
    for j, k in enumerate(dims):
        n = y.shape[k]
        gbits |= (idx[k] > (n - 1) // 2).astype(np.int64) << j
        nplanes += ((n % 2 == 1) & (idx[k] == n // 2)).astype(np.int64)
    coef = np.empty((B, len(miss)))
    for b in range(B):
        chi = np.where(np.array([bin(int(g) & b).count("1") & 1 for g in gbits], dtype=bool), -1.0, 1.0) \
            if len(miss) else np.empty(0)
        present = np.ones(len(miss), dtype=bool)
        for j, k in enumerate(dims):
            if (b >> j) & 1:
                present &= ~((y.shape[k] % 2 == 1) & (idx[k] == y.shape[k] // 2))
        coef[b] = np.where(present, chi * 2.0 ** (0.5 * nplanes) / np.sqrt(B), 0.0)
    S.update({"axes": axes, "miss": miss, "q": q, "coef": coef, "n_obs": int(y.size - len(miss))})
    return S


def border_blocks_multi(X, Y):
    """The border form of a multi-output GP on an incomplete grid (gpim_amd extension: vreconstructor's 'border' solver,
    DESIGN.md section 13).  X (d, n_1, ..., n_d) with NaN coordinates at the missing pixels, Y (n_1, ..., n_d, T) whose
    NaN rows are exactly those pixels (a row with any NaN output counts as missing for every task).

    Returns the dict of ``border_blocks`` with ys of shape (T, B, Nq) -- each task with 0 at the missing points in the
    adapted basis, task-major then sign pattern, as in ``reflection_blocks_multi`` -- and ones (B, Nq) = U 1_o, the
    basis change of the indicator of the OBSERVED points (the task means enter the blocks through it; unlike U 1 it has
    components in every block: ones_b = (U 1)_b - sum_j coef[b, j] e_{q[j]}); n_obs = the number of observed rows.
    Raises what ``border_blocks`` raises."""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim != X.ndim or X.shape[1:] != Y.shape[:-1]:
        raise NotImplementedError("grid completion needs coordinates of shape (d, n_1, ..., n_d) and Y of shape (n_1, ..., n_d, T)")
    T = Y.shape[-1]
    missing = np.isnan(Y).any(axis=-1)
    S = border_blocks(X, np.where(missing, np.nan, 0.0))
    Xc = np.array(np.meshgrid(*S["axes"], indexing="ij"))
    Y0 = np.where(missing[..., None], 0.0, Y)
    ones = reflection_blocks(Xc, (~missing).astype(np.float64), S["axes"])["ys"]
    S["ys"] = np.stack([reflection_blocks(Xc, Y0[..., a], S["axes"])["ys"] for a in range(T)]) if T \
        else np.empty((0,) + ones.shape)
    S["ones"] = ones
    return S


def border_flops(N, M, r):
    """Per-iteration flop model of the border form against the dense exact GP on the N - M observed points
    (DESIGN.md section 11): (F_border, F_dense) = (N^3 / 4^r + N^2 M / 2^r + N M^2 + M^3, (N - M)^3)."""
    N, M = float(N), float(M)
    return N ** 3 / 4.0 ** r + N * N * M / 2.0 ** r + N * M * M + M ** 3, (N - M) ** 3


def column_blocks(X, y):
    """The dense-by-Kronecker form of a grid whose missing points are whole columns (gpim_amd extension; DESIGN.md section
    22): a hyperspectral cube in which a pixel is either measured with its whole spectrum or missing with it, an image
    with whole rows missing.  The NaN mask of y is constant along the "complete" axes C and depends on the other, "ragged",
    axes only, so the observations are (observed ragged points) x (product of the complete axes) and the RBF covariance
    is K_s (x) K_c: J = prod n_i (i in C) exact-GP blocks of the N_s observed ragged points.

    X (d, n_1, ..., n_d): grid coordinates with NaN at the missing points, y (n_1, ..., n_d) with NaN at the same points.
    Returns a dict: ragged, complete (the axes, ascending), perm (ragged then complete) and inv (its inverse: an array in
    permuted axis order goes back with ``a.transpose(inv)``), shape, Xs (N_s, p: the observed ragged points, row-major in
    ragged-grid order), obs (their flat indices in the ragged grid), axes_c (the coordinate vectors of the complete axes),
    Y (N_s, J: complete axes fastest, C order), n_obs = N_s J.
    Raises NotImplementedError, naming the reason, when no axis is complete, when every axis is (nothing is missing: the
    Kronecker solver's case), when the observed coordinates do not form a product grid, when a complete axis is longer than
    4096 or J exceeds 65535."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    d = X.shape[0]
    if X.ndim != d + 1 or X.shape[1:] != y.shape or d < 2 or d > 4:
        raise NotImplementedError("column blocks need coordinates of shape (d, n_1, ..., n_d) and y of shape (n_1, ..., n_d), "
                                  "d = 2 .. 4")
    missing = np.isnan(y)
    if not np.array_equal(np.isnan(X).any(axis=0), missing):
        raise NotImplementedError("column blocks need the same NaN pattern in X and y")
    if not missing.any():
        raise NotImplementedError("column blocks: nothing is missing (every axis is complete: the Kronecker solver's case)")
    complete = [i for i in range(d) if (missing == np.take(missing, [0], axis=i)).all()]
    ragged = [i for i in range(d) if i not in complete]
    if not complete:
        raise NotImplementedError("column blocks: the NaN mask is constant along no axis (scattered missing points)")
    perm = ragged + complete
    p = len(ragged)
    mask_r = np.transpose(missing, perm)[(Ellipsis,) + (0,) * len(complete)]         # the mask over the ragged grid
    obs = np.flatnonzero(~mask_r.ravel())
    if obs.size == 0:
        raise NotImplementedError("column blocks: no observed point")
    rshape = tuple(y.shape[i] for i in ragged)
    cshape = tuple(y.shape[i] for i in complete)
    J = int(np.prod(cshape, dtype=np.int64))
    if max(cshape) > 4096:
        raise NotImplementedError("column blocks: a complete axis of %d points (the eigen-solver takes at most 4096)" % max(cshape))
    if J > 65535:
        raise NotImplementedError("column blocks: %d blocks (the batched engine takes at most 65535)" % J)
    Xp = np.transpose(X, [0] + [1 + i for i in perm]).reshape(d, -1, J)[:, obs, :]  # (d, N_s, J), observed points only
    for i in ragged:
        if not (Xp[i] == Xp[i][:, :1]).all():
            raise NotImplementedError("column blocks need a product grid (coordinate %d must not vary along a complete axis)" % i)
    axes_c = []
    for k, i in enumerate(complete):
        if not (Xp[i] == Xp[i][:1, :]).all():
            raise NotImplementedError("column blocks need a product grid (coordinate %d varying along axis %d only)" % (i, i))
        c = np.moveaxis(Xp[i][0].reshape(cshape), k, 0).reshape(cshape[k], -1)
        if not (c == c[:, :1]).all():
            raise NotImplementedError("column blocks need a product grid (coordinate %d varying along axis %d only)" % (i, i))
        axes_c.append(c[:, 0].copy())
    Xs = np.ascontiguousarray(Xp[ragged, :, 0].T)
    # ragged coordinate k must vary along ragged axis k only, where observed (as complete_grid checks)
    ridx = np.unravel_index(obs, rshape)
    for k, i in enumerate(ragged):
        ref = np.full(rshape[k], np.nan)
        ref[ridx[k]] = Xs[:, k]
        if not (ref[ridx[k]] == Xs[:, k]).all():
            raise NotImplementedError("column blocks need a product grid (coordinate %d varying along axis %d only)" % (i, i))
    Y = np.ascontiguousarray(np.transpose(y, perm).reshape(-1, J)[obs])
    return {"ragged": ragged, "complete": complete, "perm": perm, "inv": [int(k) for k in np.argsort(perm)],
            "shape": tuple(y.shape), "Xs": Xs, "obs": obs, "axes_c": axes_c, "Y": Y, "n_obs": int(obs.size) * J}


def column_flops(Ns, J):
    """Per-iteration flop model of the dense-by-Kronecker blocks, in the units of ``border_flops``:
    J N_s^3 against the dense exact GP's (J N_s)^3."""
    return float(J) * float(Ns) ** 3


def pathwise_grid(Xgrid, Xrows):
    """What a pathwise posterior draw needs from its test grid and its training rows (gpim_amd extension: reconstructor.
    sample(method='pathwise')).

    Xgrid (d, n_1, ..., n_d): the test grid, a complete product grid (what ``get_full_grid`` returns) with at least one axis
    whose coordinates are symmetric about their centre; Xrows (N, d): the training rows, each of which must coincide exactly
    with a grid point.  Returns a dict: axes (the d coordinate vectors), shape (n_1, ..., n_d), mask (bit k: axis k is
    reflected), twoc (first + last coordinate per axis, 4 entries), dims (the reflected axes), idx (int64, N): the flat
    (row-major) grid index of every training row.
    Raises NotImplementedError, naming the reason, when the grid is not a product grid, when it has no symmetric axis, when
    a training row is not on it or when two training rows are the same grid point."""
    Xgrid = np.asarray(Xgrid, dtype=np.float64)
    Xrows = np.asarray(Xrows, dtype=np.float64)
    d = Xgrid.shape[0]
    if Xgrid.ndim != d + 1:
        raise NotImplementedError("pathwise draws need a product grid: coordinates of shape (d, n_1, ..., n_d), got %s"
                                  % (Xgrid.shape,))
    axes = []
    for i in range(d):
        c = np.moveaxis(Xgrid[i], i, 0).reshape(Xgrid.shape[1 + i], -1)[:, 0].copy()
        shape = [1] * d
        shape[i] = -1
        if not np.array_equal(Xgrid[i], np.broadcast_to(c.reshape(shape), Xgrid.shape[1:])):
            raise NotImplementedError("pathwise draws need a product grid: coordinate %d does not vary along axis %d only"
                                      % (i, i))
        if len(np.unique(c)) != len(c):
            raise NotImplementedError("pathwise draws need a product grid: axis %d repeats a coordinate" % i)
        axes.append(c)
    mask, twoc, dims = 0, [0.0] * 4, []
    for k, c in enumerate(axes):         # the rule of reflection_blocks
        if len(c) >= 2 and np.allclose(c + c[::-1], c[0] + c[-1], rtol=0, atol=1e-12 * max(1.0, abs(c[-1]), abs(c[0]))):
            mask |= 1 << k
            twoc[k] = float(c[0] + c[-1])
            dims.append(k)
    if not dims:
        raise NotImplementedError("pathwise draws need a grid with at least one axis that is symmetric about its centre "
                                  "(no symmetric axis: the prior has no reflection blocks)")
    if Xrows.ndim != 2 or Xrows.shape[1] != d:
        raise NotImplementedError("pathwise draws need training rows of shape (N, %d), got %s" % (d, Xrows.shape))
    sub = []
    for k, c in enumerate(axes):
        order = np.argsort(c, kind="stable")
        pos = np.clip(np.searchsorted(c[order], Xrows[:, k]), 0, len(c) - 1)
        hit = order[pos]
        off = np.flatnonzero(c[hit] != Xrows[:, k])
        if len(off):
            raise NotImplementedError("pathwise draws need every training row on the test grid: row %d is not on it "
                                      "(coordinate %d = %r)" % (off[0], k, Xrows[off[0], k]))
        sub.append(hit)
    idx = np.ravel_multi_index(tuple(sub), Xgrid.shape[1:]).astype(np.int64)
    if len(np.unique(idx)) != len(idx):
        raise NotImplementedError("pathwise draws need distinct training rows: two of them are the same grid point")
    return {"axes": axes, "shape": tuple(Xgrid.shape[1:]), "mask": mask, "twoc": twoc, "dims": dims, "idx": idx}
