"""Cell-local solvers: mirror of python/dolfinx_eqlb/lsolver (projection.py, lsolver.py); primal.py: the statement of
the P_p Poisson solve on the device (cpp.PrimalPoisson)."""

from .primal import PoissonOperator, load_table, neumann_load, stiffness_table
from .projection import PrimalFlux, PrimalStress, embed_dg, local_projection

__all__ = ["local_projection", "embed_dg", "PrimalFlux", "PrimalStress", "PoissonOperator", "neumann_load",
           "stiffness_table", "load_table"]
