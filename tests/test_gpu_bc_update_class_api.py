"""FluxEqlbSE / FluxEqlbEV with a `fluxbc` whose callable reads a mutable time: `update_boundary_values()`
(`BoundaryData.update`) evaluates the conditions again and pushes the facet DOFs to the device handle in place; the
result is that of an equilibrator constructed at the new time."""

import numpy as np
import pytest

from dolfinx_eqlb_amd.mesh import create_unit_square
from synthetic import facet_types, make_compatible_data
from cases import BCS
from test_inhomogeneous_bc import w_lin

pytestmark = pytest.mark.gpu


class Clock:
    t = 0.0


def problem(k):
    mesh = create_unit_square(6, shuffle_seed=5, perturb=0.3)
    ft = facet_types(mesh, BCS["neumann_lt"])
    clock = Clock()

    def w_t(x, y):
        wx, wy = w_lin(x, y)
        return (1.0 + clock.t) * wx, (1.0 + clock.t) * wy

    clock.t = 1.0
    G, f = make_compatible_data(mesh, k, ft, neumann_flux=w_t)  # compatible with the values at t = 1
    clock.t = 0.0
    bf = mesh.boundary_facets()
    return mesh, clock, w_t, G, f, bf[ft[0][bf] == 1], bf[ft[0][bf] == 2]


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("cls", ["FluxEqlbSE", "FluxEqlbEV"])
def test_update_boundary_values(cls, k):
    from dolfinx_eqlb_amd import eqlb
    Eq = getattr(eqlb, cls)
    mesh, clock, w_t, G, f, prime, dual = problem(k)

    def equilibrator():
        e = Eq(k, mesh, [f], [G])
        e.set_boundary_conditions([prime], [[eqlb.fluxbc(w_t, dual)]])
        return e

    def flux(e):
        x = e.get_reconstructed_fluxes(0)
        return np.array(x[0] if cls == "FluxEqlbSE" else x, copy=True)

    # a handle exists: t = 0 equilibrated, then the step to t = 1
    stepped = equilibrator()
    stepped.equilibrate_fluxes()
    x0, b0 = flux(stepped), stepped.list_bfunctions[0].copy()
    early = equilibrator()  # no handle yet when the values change
    clock.t = 1.0
    stepped.update_boundary_values()
    stepped.list_flux[:] = 0.0  # the result is accumulated, like the reference's
    stepped.equilibrate_fluxes()
    early.boundary_data.update()
    early.equilibrate_fluxes()
    fresh = equilibrator()
    fresh.equilibrate_fluxes()
    ref = flux(fresh)
    assert np.abs(b0).max() > 0 and np.array_equal(fresh.list_bfunctions[0], 2.0 * b0)
    for name, e in (("stepped", stepped), ("early", early)):
        assert np.array_equal(e.list_bfunctions[0], fresh.list_bfunctions[0]), name
        err = np.abs(flux(e) - ref).max() / np.abs(ref).max()
        print(f"{cls} k={k} {name}: rel. deviation from the fresh equilibrator {err:.2e}")
        assert err <= 1e-11, name
    assert np.abs(ref - x0).max() > 1e-3 * np.abs(x0).max()
    # and back: the step is not a one-way street
    clock.t = 0.0
    stepped.update_boundary_values()
    stepped.list_flux[:] = 0.0
    stepped.equilibrate_fluxes()
    assert np.array_equal(stepped.list_bfunctions[0], b0)
    assert np.abs(flux(stepped) - x0).max() <= 1e-11 * np.abs(x0).max()


def test_update_needs_boundary_conditions():
    from dolfinx_eqlb_amd import eqlb
    mesh, clock, w_t, G, f, prime, dual = problem(1)
    for Eq in (eqlb.FluxEqlbSE, eqlb.FluxEqlbEV):
        with pytest.raises(RuntimeError, match="Boundary conditions have not been set"):
            Eq(1, mesh, [f], [G]).update_boundary_values()
