"""
gpim_amd -- MI355X-native engine for GPim's exact-GP reconstruction / Bayesian-optimisation
hot path.  Same public names as the reference package root (gpim/__init__.py:1-5) for the
part that is in scope: ``reconstructor``, ``boptimizer``, ``utils``, and the exact multi-output
``vreconstructor`` (reference gpim/gpreg/vgpr.py).
"""
from . import gprutils as utils
from .gpr import reconstructor
from .skgpr import skreconstructor
from .boptim import boptimizer
from .vgpr import vreconstructor
from . import acqfunc

__all__ = ["reconstructor", "skreconstructor", "boptimizer", "vreconstructor", "utils", "acqfunc"]
__version__ = "0.1.0"
