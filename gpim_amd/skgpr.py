"""
skgpr.py -- ``skreconstructor``: GP reconstruction of fully observed 2D / 3D / 4D grids with a
structured covariance.

Takes the ROLE of the reference's gpim/gpreg/skgpr.py:21-448 (``gpim.skreconstructor``): a reconstructor
for complete images / cubes that exploits the lattice structure of the inputs instead of paying the dense
O(N^3).  The reference does it with GPyTorch's structured kernel interpolation (an approximation, with
GPyTorch's own hyper-parameter parameterisation: constant mean, softplus-constrained scale and noise);
this engine does it EXACTLY -- for the RBF kernel through the Kronecker factorisation of the covariance
(csrc/kron.hip), for 'Matern52' (the reference's other structured kernel, gpim/kernels/gpytorch_kernels.py:65) and
'RationalQuadratic' through the reflection symmetry of the complete grid (2^r dense blocks of N / 2^r points,
gprutils.reflection_blocks + csrc/engine.hip: kmat_refl_kernel) -- with the model and parameterisation of
``gpim_amd.reconstructor`` (zero mean, Uniform priors on variance and lengthscales).  Same constructor shape and return values as the reference class;
numbers are those of ``reconstructor(..., structured=True)``, i.e. of the exact GP -- not bit-comparable
with an SKI run.  ``kernel='Spectral'`` (GPyTorch's spectral-mixture kernel, for which the reference turns SKI off) returns
the exact GP of gpim_amd/smgpr.py on the observed points of any grid, sparse images included; complete and nearly complete
grids run there as reflection blocks too (``rec.solver``).  Incomplete grids (NaN in y)
with the other kernels: the exact GP on the observed points, either as the reflection blocks of the completed grid with a
border for the missing points (csrc/border.hip) or on the dense engine, whichever the flop model says is cheaper
(``rec.solver``: 'border' or 'dense').  With the RBF kernel, a grid whose missing points are whole columns -- a
hyperspectral cube measured at a sparse set of pixels, an image with whole rows missing -- is an exact Kronecker product of
the observed pixels and the complete axes: J dense blocks of the N_s observed pixels (gprutils.column_blocks, csrc/pkron.hip;
``rec.solver``: 'columns') instead of one of J N_s points.
"""
import numpy as np

from . import gprutils
from .gpr import reconstructor

# the border form is chosen when its flop model is below this fraction of the dense model's (at a
# model ratio of 0.74 the border still ran 1.14x (128 x 128) and 1.31x (256 x 256) faster than dense)
BORDER_FACTOR = 0.75


class skreconstructor(reconstructor):
    """``skreconstructor(X, y, Xtest=None, kernel='RBF', lengthscale=None, ski=True, learning_rate=.1,
    iterations=50, use_gpu=1, verbose=1, seed=0, **kwargs)`` -- argument order and defaults of
    gpim/gpreg/skgpr.py:79-91.  ``ski``, ``grid_points_ratio``, ``max_root``, ``num_batches`` are accepted
    and ignored (nothing is interpolated or batched), and so is ``sparse``; ``kernel``: 'RBF', 'Matern52', 'RationalQuadratic',
    or 'Spectral' (then the object is a ``gpim_amd.smgpr.smreconstructor``)."""

    def __new__(cls, X, y, Xtest=None, kernel='RBF', *args, **kwargs):
        if kernel == 'Spectral':
            from .smgpr import smreconstructor
            return smreconstructor(X, y, Xtest, kernel, *args, **kwargs)
        return super().__new__(cls)

    def __init__(self, X, y, Xtest=None, kernel='RBF', lengthscale=None, ski=True, learning_rate=.1,
                 iterations=50, use_gpu=1, verbose=1, seed=0, **kwargs):
        for k in ("grid_points_ratio", "max_root", "maxroot", "num_batches", "n_mixtures", "sparse", "_border",
                  "_columns"):
            kwargs.pop(k, None)
        solver, blocks = self._choose_solver(X, y, kernel)
        super().__init__(X, y, Xtest, kernel=kernel, lengthscale=lengthscale, sparse=False, indpoints=None,
                         learning_rate=learning_rate, iterations=iterations, use_gpu=use_gpu, verbose=verbose,
                         seed=seed, structured=solver != "dense", _border=blocks if solver == "border" else None,
                         _columns=blocks if solver == "columns" else None, **kwargs)
        self.solver = solver

    def ivr(self, *args, **kwargs):
        raise NotImplementedError("ivr(): integrated variance reduction belongs to the dense exact GP of reconstructor; "
                                  "skreconstructor models grids through structured solvers")

    ivr_batch = ivr

    def acq_batch(self, *args, **kwargs):
        raise NotImplementedError("acq_batch(): believer batches belong to the dense exact GP of reconstructor; "
                                  "skreconstructor models grids through structured solvers")

    @staticmethod
    def _choose_solver(X, y, kernel):
        """('kronecker' | 'reflection', None) on a complete grid; on an incomplete one ('border', border_blocks(X, y)) when
        the grid can be completed, has a symmetric axis and the border's flop model is below BORDER_FACTOR of the dense
        exact GP's on the observed points, else ('dense', None).  RBF on a grid whose missing points are whole columns:
        ('columns', column_blocks(X, y)) when the blocks' flop model is below that of the choice above."""
        yv = np.asarray(y, dtype=np.float64)
        if not np.isnan(yv).any():
            return ("kronecker" if kernel == "RBF" else "reflection"), None
        if kernel not in ("RBF", "Matern52", "RationalQuadratic"):
            return "dense", None
        n_obs = int(np.count_nonzero(~np.isnan(yv)))
        choice, f_choice = ("dense", None), float(n_obs) ** 3
        try:
            S = gprutils.border_blocks(X, yv)
            f_border, f_dense = gprutils.border_flops(yv.size, len(S["miss"]), len(S["dims"]))
            if f_border < BORDER_FACTOR * f_dense:
                choice, f_choice = ("border", S), f_border
        except (NotImplementedError, ValueError):
            pass
        if kernel == "RBF":
            try:
                C = gprutils.column_blocks(X, yv)
            except NotImplementedError:
                return choice
            if gprutils.column_flops(C["Xs"].shape[0], C["Y"].shape[1]) < f_choice:
                return "columns", C
        return choice
