"""
_sampling.py -- the host side of posterior draws: one driver for the six methods of ``reconstructor.sample``, and the pieces
``vreconstructor.sample`` shares with it (DESIGN.md sections 16-19, 21, 23).

``draw`` takes every method through the same steps in the same order: the method's gate (is this the engine it is built
for), ``_check_data``, the test grid resolved WITHOUT storing it (finite, or ValueError), the method's geometry on that
grid, ``n_samples``, the shape of a given ``z``, the jitter rule, device memory -- and only then stores a new grid, draws
``z`` when none was given, allocates, calls the solver and remembers the size of the call.  So a refused call leaves the
model, its stored test grid and the solver's test axes as they were, whatever the method.  ``draw_device`` is the same for
device rows and a device ``z`` (Thompson sampling, acqfunc.thompson_on_device).  ``SPECTRAL_METHODS`` are the three methods of
``skreconstructor(kernel='Spectral').sample``: the same objects with their gate, the source of the
jitter rule's noise and their call replaced, through the same ``draw``.

A method says what differs (``o`` is the reconstructor): ``gate(o)``; ``grid(o, Xtest) -> (X, shape)``, rows on the device
or the coordinate vectors of a product grid; ``geometry(o, X, shape) -> g``, a dict of host sizes and of what the call
takes; ``plan(g, S, noiseless, z_on_device) -> (W, layout, bytes, subject)``, the width of z, the words for its layout, the
device memory of the call and the subject of its MemoryError, from ``g`` alone (no device); ``jitter``, a rule of
``_check_jitter``, with ``jitter_default(o)`` and ``jitter_bound(o)`` (the noise plus the model's own jitter, named by
``BOUND``); ``call(o, g, X, z, noiseless, jitter, mean, out) -> rc``.
"""
import numpy as np
import torch

from . import _lib, _solvers, gprutils

_F64 = torch.float64
FINITE = "sample: the test grid must be finite (NaN rows have no joint distribution)"


def factor_bytes(n):
    """Bytes of the square workspace in which the library factors a matrix of order n: the order padded to a multiple of
    128, rows of 1024 entries and more set 16 entries apart from a power of two."""
    order = -(-int(n) // 128) * 128
    return order * (order + (16 if order >= 1024 else 0)) * 8


def block_points(P):
    """The points of one reflection block of the grid P (gprutils.pathwise_grid): M / 2^r for axes of even length."""
    return int(np.prod([(n + 1) // 2 if k in P["dims"] else n for k, n in enumerate(P["shape"])]))


def reserve(o, method, need, subject, of_total=False):
    """MemoryError unless `need` bytes are free on the device or a call of this method and size has run on this model (the
    handle keeps its workspaces, grow-only)."""
    if need > o._draw_bytes.get(method, 0):
        free, total = torch.cuda.mem_get_info(o._dev)
        if need > free:
            left = "%.2f of %.2f" % (free / 2.0 ** 30, total / 2.0 ** 30) if of_total else "%.2f" % (free / 2.0 ** 30)
            raise MemoryError("sample: %s %.2f GiB of device memory, %s GiB are free" % (subject, need / 2.0 ** 30, left))


def record(o, method, need):
    o._draw_bytes[method] = max(need, o._draw_bytes.get(method, 0))


def rows_grid(Xtest, prepare, stored, default):
    """(rows, grid shape) of a call's test grid, nothing stored: ``prepare(Xtest)`` of a given grid (finite, or ValueError),
    else the pair `stored` when the model holds a grid, else `default`."""
    if Xtest is None:
        return default if stored[0] is None else stored
    if not np.isfinite(np.asarray(Xtest, dtype=np.float64)).all():
        raise ValueError(FINITE)
    return prepare(Xtest), tuple(Xtest.shape[1:])


def require_finite(o, rows_d):
    """ValueError unless the device rows are finite; one device-to-host look per tensor (boptimizer draws on the same grid at
    every step)."""
    if getattr(o, "_finite_rows", None) is not rows_d:
        if not bool(torch.isfinite(rows_d).all()):
            raise ValueError(FINITE)
        o._finite_rows = rows_d


def _device_rows(o, Xtest, default):
    X, shape = rows_grid(Xtest, lambda Xt: o._to_device(gprutils.prepare_test_data(Xt, precision=o.precision)),
                         (o._Xtest_d, tuple(o.fulldims)), default)
    if X is not None:
        require_finite(o, X)
    return X, shape


def _product_axes(o, Xtest, name, stored):
    """(the d coordinate vectors, grid shape) of a product test grid: Xtest's, else those the solver holds."""
    if Xtest is None:
        if stored is None:
            raise NotImplementedError("method='%s' needs a product test grid: the model holds none (pass Xtest)" % name)
        if not all(np.isfinite(t).all() for t in stored):
            raise ValueError(FINITE)
        return stored, tuple(o.fulldims)
    if not np.isfinite(np.asarray(Xtest, dtype=np.float64)).all():
        raise ValueError(FINITE)
    try:
        return gprutils.grid_axes(Xtest)[0], tuple(np.shape(Xtest)[1:])
    except NotImplementedError as e:
        raise NotImplementedError("method='%s' needs a product test grid: %s" % (name, e))


def _union_cap(name, union_axes, axis_names):
    for i, a in zip(axis_names, union_axes):
        if len(a) > 4096:
            raise NotImplementedError("method='%s': the union of the training and the test coordinates of axis %d has %d "
                                      "entries, the eigen-solver takes at most 4096" % (name, i, len(a)))


def _refuse(engine, *reasons):
    """NotImplementedError(engine % why) for the first (condition, why) that holds."""
    for cond, why in reasons:
        if cond:
            raise NotImplementedError(engine % why)


def _noise(noiseless):
    return "" if noiseless else ", noise on the grid"


class Joint:
    """One factorisation of the (N + M)^2 joint covariance, at any finite rows (csrc/sample.hip); z is (S, M)."""
    name, jitter, checks_n_samples, memory_of_total = "joint", None, False, False
    stores_training_grid = True     # without any test grid the training points become the stored one, as in predict()
    ENGINE = "joint posterior draws are built for the dense double-precision engine only (%s)"
    BOUND = "noise + the model's jitter"

    def jitter_default(self, o):
        return o._spec.jitter

    def jitter_bound(self, o):
        return float(o._spec.constrained(o._u)[2]) + o._spec.jitter

    def gate(self, o):
        _refuse(self.ENGINE, (o.do_sparse, "sparse=True"), (o.do_structured or o.do_symm, "structured=True"),
                (o.precision == "single", "precision='single'"))

    def grid(self, o, Xtest):
        return _device_rows(o, Xtest, (o._Xd, tuple(o.fulldims)))

    def geometry(self, o, X, shape):
        return {"N": o._Xd.shape[0], "M": X.shape[0]}

    def plan(self, g, S, noiseless, z_on_device):
        return (g["M"], "", factor_bytes(g["N"] + g["M"]),
                "the joint covariance of %d training and %d test points needs" % (g["N"], g["M"]))

    def device_layout(self, g, noiseless):
        return ""

    def call(self, o, g, X, z, noiseless, jitter, mean, out):
        g["var"] = torch.empty_like(mean)
        return o._solver.sample(o, X, z, noiseless, jitter, mean, g["var"], out)


class Pathwise(Joint):
    """Matheron's rule on a complete product grid that holds every training row; z is
    [z_p (M) | z_e (N) | z_n (M, unless noiseless)]."""
    name, jitter = "pathwise", ("noise", "pathwise draws need")

    def geometry(self, o, X, shape):
        """The dict of gprutils.pathwise_grid and its idx on the device, kept while the grid rows and the training rows stay
        the same tensors."""
        c = getattr(o, "_pw_cache", None)
        if c is None or c[0] is not X or c[1] is not o._Xd or c[2] != tuple(shape):
            d = o._Xd.shape[1]
            if len(shape) != d or int(np.prod(shape)) != X.shape[0]:
                raise NotImplementedError("pathwise draws need a product grid: %d test rows do not fill a grid of shape %s in "
                                          "%d dimensions" % (X.shape[0], tuple(shape), d))
            P = gprutils.pathwise_grid(X.cpu().numpy().T.reshape((d,) + tuple(shape)), o._Xd.cpu().numpy())
            c = o._pw_cache = (X, o._Xd, tuple(shape), P, torch.from_numpy(P["idx"]).to(o._dev))
        return {"N": o._Xd.shape[0], "M": X.shape[0], "P": c[3], "idx_d": c[4], "nq": block_points(c[3])}

    def plan(self, g, S, noiseless, z_on_device):
        # one (M / 2^r)^2 block of the prior and the N^2 training covariance
        return (g["M"] + g["N"] + (0 if noiseless else g["M"]), "", factor_bytes(g["nq"]) + factor_bytes(g["N"]),
                "a prior block of %d points and the covariance of %d training points need" % (g["nq"], g["N"]))

    def device_layout(self, g, noiseless):
        return " for method='pathwise' (M = %d grid points, N = %d observations%s)" % (g["M"], g["N"], _noise(noiseless))

    def call(self, o, g, X, z, noiseless, jitter, mean, out):
        return o._solver.sample_pathwise(o, X, g["P"], g["idx_d"], z, noiseless, jitter, mean, out)


class Blocks(Pathwise):
    """The pathwise draw for observations on every grid point, in the grid's reflection basis alone:
    the test grid must be the training grid; z as for 'pathwise' with N = M."""
    name, jitter, stores_training_grid = "blocks", ("noise", "method='blocks' needs"), False
    ENGINE = "method='blocks' draws on a fully observed grid in double precision (%s)"

    def gate(self, o):
        _refuse(self.ENGINE, (o.do_sparse, "sparse=True"), (o.precision == "single", "precision='single'"),
                (o.do_border, "the image has missing points: method='blocks' needs a fully observed grid"))

    def geometry(self, o, X, shape):
        g = Pathwise.geometry(self, o, X, shape)
        N, M, P = g["N"], g["M"], g["P"]
        if N != M:          # (distinct rows, each on the grid: fewer of them than grid points)
            first = int(np.setdiff1d(np.arange(M), P["idx"])[0])
            raise NotImplementedError("method='blocks' needs an observation on every point of the test grid (the test grid "
                                      "must be the training grid): grid point %s has none (%d observations, %d grid points)"
                                      % (tuple(int(v) for v in np.unravel_index(first, shape)), N, M))
        g["P"] = dict(P, idx_d=None if np.array_equal(P["idx"], np.arange(M)) else g["idx_d"])
        return g

    def plan(self, g, S, noiseless, z_on_device):
        # one (M / 2^r)^2 reflection block, reused by all the factorisations
        return (2 * g["M"] + (0 if noiseless else g["M"]),
                " for method='%s' (M = %d grid points%s)" % (self.name, g["M"], _noise(noiseless)),
                factor_bytes(g["nq"]), "a reflection block of %d points needs" % g["nq"])

    def call(self, o, g, X, z, noiseless, jitter, mean, out):
        return o._solver.sample_blocks(o, X, g["P"], z, noiseless, jitter, mean, out)


class Border(Blocks):
    """The pathwise draw for an image with missing pixels through the bordered reflection blocks of the completed grid,
    which must be the test grid; z as for 'blocks', every part indexed by the grid point."""
    name, jitter, memory_of_total = "border", ("noise", "method='border' needs"), True
    ENGINE = "method='border' draws on an image with missing points through its bordered reflection blocks, in " \
             "double precision (%s)"

    def gate(self, o):
        _refuse(self.ENGINE, (o.do_sparse, "sparse=True"), (o.precision == "single", "precision='single'"),
                (not o.do_border and (o.do_symm or o.do_structured), "the grid is fully observed: use method='blocks'"),
                (not o.do_border, "a dense model: use method='pathwise', or skreconstructor for an image or cube with "
                                  "missing pixels"))

    def grid(self, o, Xtest):
        return _device_rows(o, Xtest, (None, tuple(len(c) for c in o._solver.S["axes"])))

    def geometry(self, o, X, shape):
        """The completed grid's rows and the missing points' indices on the device, kept; a given grid must equal it."""
        B = o._solver.S
        gshape = tuple(len(c) for c in B["axes"])
        c = getattr(o, "_border_grid", None)
        if c is None:
            G = np.array(np.meshgrid(*B["axes"], indexing="ij")).reshape(len(gshape), -1).T
            c = o._border_grid = [o._to_device(np.ascontiguousarray(G)),
                                  torch.from_numpy(B["miss"].astype(np.int64)).to(o._dev), None]
        if X is not None and c[2] is not X:
            if shape != gshape or X.shape != c[0].shape or not bool(torch.equal(X, c[0])):
                raise NotImplementedError("method='border' needs the completed training grid as its test grid (Xtest None, the "
                                          "stored grid, or a grid equal to it: shape %s); got a grid of shape %s that is not it"
                                          % (gshape, shape))
            if X is o._Xtest_d:
                c[2] = X                    # the stored grid: compared once
        return {"M": c[0].shape[0], "nq": B["Xq"].shape[0], "G_d": c[0], "miss_d": c[1],
                "P": {"shape": gshape, "mask": B["mask"], "twoc": B["twoc"]}}

    def call(self, o, g, X, z, noiseless, jitter, mean, out):
        return o._solver.sample_border(o, g["G_d"], g["P"], g["miss_d"], z, noiseless, jitter, mean, out)


class Kron:
    """Matheron's rule with every factor a Kronecker product, on any finite product grid; z is
    [zeta (prod U_i) | z_e (N) | z_n (M)] whether noiseless or not."""
    name, stores_training_grid, checks_n_samples, memory_of_total = "kron", False, True, False
    jitter = ("ge0", "method='kron' needs a finite jitter >= 0")
    jitter_default = Joint.jitter_default
    ENGINE = "method='kron' draws through the Kronecker eigenbasis: reconstructor(..., kernel='RBF', structured=True) " \
             "or skreconstructor(..., 'RBF') on a fully observed grid, in double precision (%s)"

    def gate(self, o):
        _refuse(self.ENGINE, (o.do_sparse, "sparse=True"), (o.do_border, "the image has missing points: use method='border'"),
                (o.do_symm, "a reflection-block model: use method='blocks'"),
                (not isinstance(o._solver, _solvers.Kron), "a dense model: use method='joint' or 'pathwise'"),
                (o.precision == "single", "precision='single'"))

    def grid(self, o, Xtest):
        return _product_axes(o, Xtest, "kron", o._solver.taxes[0])

    def geometry(self, o, taxes, shape):
        return self.sizes(o._solver.axes, taxes)

    def sizes(self, axes, taxes):
        """g of the training axes and the test axes: host arithmetic only."""
        union = gprutils.union_axes(axes, taxes)
        _union_cap("kron", union[0], range(len(axes)))
        nu, nn, nm = [len(a) for a in union[0]], [len(c) for c in axes], [len(t) for t in taxes]
        PU, N, M = (int(np.prod(n, dtype=np.int64)) for n in (nu, nn, nm))
        # what the library allocates (csrc/kron.hip): per draw zeta and the two buffers of the mode products (the largest tensor a
        # chain of mode products passes through); once the gathered root rows, the union axes' matrices when the training
        # decomposition does not serve, and the prediction workspace
        smax, pmax = max(N, M), N
        for src, dst in ((nu, nn), (nu, nm), (nn, nm)):
            cur = int(np.prod(src, dtype=np.int64))
            for a, b in zip(src, dst):
                cur = cur // a * b
                smax = max(smax, cur)
                if src is nn:
                    pmax = max(pmax, cur)
        shared = nu == nn and all(np.array_equal(i, np.arange(len(i))) for i in union[1])
        lib_axes = 0 if shared else 2 * sum(nu) + 5 * sum(a * a for a in nu)
        lib_rows = sum((a + b) * c for a, b, c in zip(nn, nm, nu))
        lib_pred = sum(nm) + 2 * sum(a * b for a, b in zip(nn, nm)) + 2 * pmax
        return {"PU": PU, "N": N, "M": M, "union": union, "per_draw": M + PU + 2 * smax,
                "once": M + lib_axes + lib_rows + lib_pred}

    def plan(self, g, S, noiseless, z_on_device):
        W = g["PU"] + g["N"] + g["M"]
        # z, the draws and the mean here, and the library's buffers
        return (W, " for method='kron' ([zeta | z_e | z_n] = %d union-grid points + %d observations + %d test points)"
                % (g["PU"], g["N"], g["M"]), 8 * (S * ((0 if z_on_device else W) + g["per_draw"]) + g["once"]),
                "%d draws on %d test points through %d union-grid points need" % (S, g["M"], g["PU"]))

    def call(self, o, g, taxes, z, noiseless, jitter, mean, out):
        return o._solver.sample_kron(o, taxes, g["union"], z, noiseless, jitter, mean, out)


class Columns:
    """Matheron's rule through the dense-by-Kronecker blocks of a cube with missing spectra, on any finite product grid
    (DESIGN.md section 23); z is [zeta (U_s prod U_i) | z_e (N) | z_n (M)] whether noiseless or not."""
    name, stores_training_grid, checks_n_samples, memory_of_total = "columns", False, True, False
    jitter = ("gt0", "method='columns' needs a finite jitter > 0 (the prior factor of the ragged rows)")
    jitter_default = Joint.jitter_default
    ENGINE = "method='columns' draws through the dense-by-Kronecker blocks: skreconstructor(..., 'RBF') whose solver " \
             "is 'columns' (whole columns of the grid missing), in double precision (%s)"

    def gate(self, o):
        _refuse(self.ENGINE, (o.do_sparse, "sparse=True"), (o.do_border, "the missing points are scattered: use method='border'"),
                (isinstance(o._solver, _solvers.Kron), "the Kronecker model of a complete grid: use method='kron'"),
                (o.do_symm, "a reflection-block model: use method='blocks'"),
                (not isinstance(o._solver, _solvers.Columns), "a dense model: use method='joint' or 'pathwise'"),
                (o.precision == "single", "precision='single'"))

    def grid(self, o, Xtest):
        return _product_axes(o, Xtest, "columns", o._solver.taxes)

    def geometry(self, o, taxes, shape):
        return self.sizes(o._solver, taxes)

    def sizes(self, sol, taxes):
        """g of the column-blocks solver and the test axes: host arithmetic only."""
        geometry = sol.sample_geometry(taxes)
        rows, caxes, (P, _, _), (au, _, _) = geometry
        _union_cap("columns", au, sol.C["complete"])
        Ns, J = sol.C["Y"].shape
        return {"Us": len(P), "U": int(np.prod([len(a) for a in au], dtype=np.int64)), "N": sol.C["n_obs"],
                "M": int(np.prod([len(t) for t in taxes], dtype=np.int64)), "geometry": geometry,
                "library": (Ns, len(rows), len(P), J, [len(a) for a in au], [len(c) for c in sol.C["axes_c"]],
                            [len(c) for c in caxes])}

    def plan(self, g, S, noiseless, z_on_device):
        Us, U, N, M = g["Us"], g["U"], g["N"], g["M"]
        W = Us * U + N + M
        # z (as given and in the library's layout), the draws twice and the mean here; in the library (csrc/pkrongp.hip:
        # gpimhip_sample_pkron) the prior factor, zeta and H, the mode products' and the blocks' buffers
        need = 8 * (S * ((1 if z_on_device else 2) * W + 2 * M) + 2 * M + _columns_library_doubles(S, *g["library"]))
        return (W, " for method='columns' ([zeta | z_e | z_n] = %d x %d union rows x union-axes points + %d observations + %d "
                "test points)" % (Us, U, N, M), need,
                "%d draws on %d test points through %d x %d union points need" % (S, M, Us, U))

    def call(self, o, g, taxes, z, noiseless, jitter, mean, out):
        return o._solver.sample_columns(o, taxes, z, noiseless, jitter, mean, out, g["geometry"])


def _columns_library_doubles(S, Ns, Ms, Us, J, nu, nn, nm):
    """The doubles gpimhip_sample_pkron's own buffers take (its arena and the prediction slab), by the library's formulas."""
    pad = lambda n: -(-int(n) // 128) * 128
    np_, npU = pad(Ns), pad(Us)
    nb = np_ // 128
    mc = min(pad(Ms), max(128, (1 << 26) // (J * nb) // 128 * 128))
    U = int(np.prod(nu, dtype=np.int64))
    pmax, cur, cx, ct, maxX, maxT = 1, J, U, U, U, U
    for a, b, c in zip(nu, nn, nm):
        cur, cx, ct = cur // b * c, cx // a * b, ct // a * c
        pmax, maxX, maxT = max(pmax, cur), max(maxX, cx), max(maxT, ct)
    big = max(Ns * maxX, Ms * maxT)
    per_draw = 2 * npU * U + 3 * big + 2 * pmax * mc + J * (3 * np_ + mc)
    sg = max(1, min(S, (1 << 25) // per_draw))
    groups = -(-S // sg)
    sg = -(-S // groups)
    cols, Sp, rowsP = pad(sg * U), pad(sg), pad(sg * J)
    arena = npU * (npU + 16) + 2 * npU * cols + 3 * sg * big + 2 * J * np_ * Sp + rowsP * (np_ + mc) + 2 * sg * pmax * mc
    slab = np_ * (mc + 16) + nb * mc + pad(J) * mc + 4 * pmax * mc
    return arena + slab


METHODS = {m.name: m() for m in (Joint, Pathwise, Blocks, Border, Kron, Columns)}


class _Spectral:
    """What differs for ``smreconstructor``.  A method is gated by the data, not by ``rec.solver``:
    the posterior depends on the observed rows and u only, which every solver's model holds.  The model has no jitter of
    its own, so the jitter rule's bound is the noise, and the draw's jitter defaults to 1e-5 (below the noise floor 1e-4)."""
    BOUND = "noise (this model has no jitter of its own)"

    def gate(self, o):
        pass

    def jitter_default(self, o):
        return 1e-5

    def jitter_bound(self, o):
        return o._params()[4]

    @staticmethod
    def phase_bytes(o, *rows):
        """The phase buffers of the library: 2 Q d doubles per row, the rows padded to 128 per buffer."""
        return 16 * o.num_mixtures * o._Xd.shape[1] * sum(-(-int(n) // 128) * 128 for n in rows)


class SpectralJoint(_Spectral, Joint):
    jitter = ("ge0", "method='joint' needs a finite jitter >= 0")

    def geometry(self, o, X, shape):
        return dict(Joint.geometry(self, o, X, shape), phases=self.phase_bytes(o, o._Xd.shape[0] + X.shape[0]))

    def plan(self, g, S, noiseless, z_on_device):
        W, layout, need, subject = Joint.plan(self, g, S, noiseless, z_on_device)
        return W, layout, need + g["phases"], subject

    def call(self, o, g, X, z, noiseless, jitter, mean, out):
        g["var"] = torch.empty_like(mean)
        return o._draw_joint(X, z, noiseless, jitter, mean, g["var"], out)


class SpectralPathwise(_Spectral, Pathwise):
    def geometry(self, o, X, shape):
        g = Pathwise.geometry(self, o, X, shape)
        return dict(g, phases=self.phase_bytes(o, g["N"], g["nq"], g["M"]))

    def plan(self, g, S, noiseless, z_on_device):
        W, layout, need, subject = Pathwise.plan(self, g, S, noiseless, z_on_device)
        return W, layout, need + g["phases"], subject

    def call(self, o, g, X, z, noiseless, jitter, mean, out):
        return o._draw_pathwise(X, g["P"], g["idx_d"], z, noiseless, jitter, mean, out)


class SpectralBlocks(_Spectral, Blocks):
    def geometry(self, o, X, shape):
        g = Blocks.geometry(self, o, X, shape)
        return dict(g, phases=self.phase_bytes(o, g["nq"]))

    def plan(self, g, S, noiseless, z_on_device):
        W, layout, need, subject = Blocks.plan(self, g, S, noiseless, z_on_device)
        return W, layout, need + g["phases"], subject

    def call(self, o, g, X, z, noiseless, jitter, mean, out):
        return o._draw_blocks(X, g["P"], z, noiseless, jitter, mean, out)


SPECTRAL_METHODS = {m.name: m() for m in (SpectralJoint, SpectralPathwise, SpectralBlocks)}


def _check_jitter(o, m, jitter):
    """The jitter of the call (default: the method's, i.e. the model's) under the method's rule: 'noise' 0 < jitter <= noise
    + the model's jitter, 'ge0' 0 <= jitter < inf, 'gt0' 0 < jitter < inf; None: the library checks it."""
    jitter = m.jitter_default(o) if jitter is None else float(jitter)
    rule, text = m.jitter or (None, None)
    if rule == "noise":
        s = m.jitter_bound(o)
        if not (0.0 < jitter <= s):
            raise ValueError("%s 0 < jitter <= %s = %g; got %g" % (text, m.BOUND, s, jitter))
    elif rule and not ((0.0 <= jitter if rule == "ge0" else 0.0 < jitter) and jitter < np.inf):
        raise ValueError("%s; got %g" % (text, jitter))
    return jitter


def _draw(o, m, X, shape, n_samples, z, noiseless, jitter, seed=None, Xtest=None):
    """The steps every call takes once its grid is resolved.  n_samples None: the device entry, z a device tensor."""
    host = n_samples is not None
    g = m.geometry(o, X, shape)
    S = int(n_samples) if host else z.shape[0]
    if host and m.checks_n_samples and S < 1:
        raise ValueError("n_samples must be at least 1; got %r" % (n_samples,))
    W, layout, need, subject = m.plan(g, S, noiseless, torch.is_tensor(z) and z.is_cuda and z.dtype == _F64)
    if z is not None and (z.ndim != 2 or tuple(z.shape) != (S, W)):
        raise ValueError("z must have shape (n_samples, %d)%s; got %s"
                         % (W, " = (%d, %d)" % (S, W) + layout if host else m.device_layout(g, noiseless), tuple(z.shape)))
    jitter = _check_jitter(o, m, jitter)
    reserve(o, m.name, need, subject, m.memory_of_total)
    if host and (Xtest is not None or m.stores_training_grid):
        o._resolve_test_grid(Xtest)
    z_d = o._draw_z(S, W, seed) if z is None else o._to_device(z)
    out = torch.empty((S, g["M"]), dtype=_F64, device=o._dev)
    mean = torch.empty((g["M"],), dtype=_F64, device=o._dev)
    _lib.check(m.call(o, g, X, z_d, noiseless, jitter, mean, out))
    record(o, m.name, need)
    return out, mean, g.get("var")


def draw_device(o, name, X, shape, z_d, noiseless, jitter):
    """(samples (S, M), mean (M), var (M) or None) device tensors of the draws of 'joint' or 'pathwise' at the device rows X
    (filling a grid of shape `shape`) with the device normals z_d (S, W)."""
    m = METHODS[name]
    m.gate(o)
    o._check_data()
    require_finite(o, X)
    return _draw(o, m, X, shape, None, z_d, noiseless, jitter)


def draw(o, name, n_samples, Xtest, noiseless, seed, z, jitter, methods=METHODS):
    """``reconstructor.sample`` (and ``smreconstructor.sample`` with ``methods=SPECTRAL_METHODS``): ndarray (n_samples, *grid
    shape) of method `name`'s draws."""
    m = methods[name]
    if name != "columns" and isinstance(o._solver, _solvers.Columns):
        raise NotImplementedError(_solvers.Columns._NO_DRAWS + " (got method=%r)" % (name,))
    m.gate(o)
    o._check_data()
    X, shape = m.grid(o, Xtest)
    if z is not None and not torch.is_tensor(z):
        z = np.asarray(z)
    out = _draw(o, m, X, shape, n_samples, z, noiseless, jitter, seed, Xtest)[0]
    return out.cpu().numpy().reshape((out.shape[0],) + shape).astype(o._np_out, copy=False)
