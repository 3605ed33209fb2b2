"""``gpim.gpreg.vgpr`` -> gpim_amd.vgpr (reference: gpim/gpreg/vgpr.py:19-283)."""
from gpim_amd.vgpr import vreconstructor          # noqa: F401
