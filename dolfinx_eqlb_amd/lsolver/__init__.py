"""Cell-local solvers: mirror of python/dolfinx_eqlb/lsolver (projection.py, lsolver.py); primal.py: the statements of
the P_p Poisson solve and the P_p^2 elasticity solve on the device (cpp.PrimalPoisson, cpp.PrimalElasticity);
multilevel.py: the statement of the multilevel preconditioner of those solves (cpp.Multilevel)."""

from .primal import (ElasticityOperator, PoissonOperator, cross_table, csr_apply, diffusion_min_eigenvalue,
                     diffusion_oscillation_weight, flux_dg_tensor, load_table, mass_table, neumann_load, stiffness_table,
                     traction_load, value_table, facet_mass_table, robin_flux, robin_load, spring_flux,
                     spring_list, spring_load, spring_tensor)
from .multilevel import Hierarchy
from .projection import PrimalFlux, PrimalStress, PrimalValue, embed_dg, local_projection

__all__ = ["local_projection", "embed_dg", "PrimalFlux", "PrimalStress", "PoissonOperator", "neumann_load",
           "stiffness_table", "load_table", "ElasticityOperator", "traction_load", "cross_table", "Hierarchy",
           "PrimalValue", "mass_table", "value_table", "flux_dg_tensor", "diffusion_min_eigenvalue",
           "diffusion_oscillation_weight", "csr_apply", "facet_mass_table", "robin_flux", "robin_load",
           "spring_flux", "spring_list", "spring_load", "spring_tensor"]
