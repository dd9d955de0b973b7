"""Weak symmetry of the stress on the bins whose dense tiles do not fit the LDS - RT_4 with patches of 9 ... 64
facets (P = 16, 32, 64) and RT_3 with 33 ... 64 facets (P = 64) - through the banded solver
(eqlb_se_weaksym_banded.hip), against the oracle restatement of the reference."""

import numpy as np
import pytest

import galerkin as gk
from cases import big_double_fan_mesh
from test_gpu_unstructured import delaunay_mesh
from test_oracle_stress import asym_moments

pytestmark = pytest.mark.gpu


def run_stress(oracle_mod, mesh, k, ft, G, f, bv=None):
    """Device stress against the oracle (rel 1e-10), weak symmetry, and a bitwise equal second call."""
    from dolfinx_eqlb_amd import cpp
    ref = oracle_mod.se_reconstruct(mesh, k, ft, G, f, boundary_values=bv, stress=True)
    eq = cpp.SemiExplicitEquilibrator(cpp.DeviceMesh(mesh), k, 2, reconstruct_stress=True)
    eq.set_boundary(ft, boundary_values=bv)
    x = eq.equilibrate_host(G, f)
    assert np.isfinite(x).all()
    scale = np.abs(ref).max()
    assert np.abs(x - ref).max() <= 1e-10 * scale
    assert np.abs(asym_moments(mesh, k, x)[1]).max() < 1e-11 * max(1.0, scale)
    assert np.array_equal(x, eq.equilibrate_host(G, f))
    return x


def disk_data(mesh, k, traction, data):
    """Dirichlet rim, or tractions on the upper half of the rim for both rows; synthetic or Galerkin data."""
    from synthetic import facet_types, make_compatible_stress_data
    if data == "synthetic":
        sel = (lambda x: x[:, 1] > 0.0) if traction else None
        ft = np.repeat(facet_types(mesh, sel), 2, axis=0)
        G, f = make_compatible_stress_data(mesh, k, ft)
        return ft, G, f, None
    ft = flux_types(mesh, [(lambda m: m[:, 1] > 0.0) if traction else None] * 2)
    G, f, bv = gk.solve_elasticity(mesh, k, ft, seed=31 * k + mesh.nnodes)
    return ft, G, f, bv


def flux_types(mesh, sels):
    """facet_type [2, nfacets]: boundary facets whose midpoint satisfies sels[r] carry a traction in row r
    (type 2), the other boundary facets a displacement condition (type 1)."""
    ft = np.zeros((2, mesh.nfacets), dtype=np.int8)
    bf = mesh.boundary_facets()
    mid = mesh.x[mesh.facet_nodes[bf]].mean(axis=1)[:, :2]
    for r in range(2):
        ft[r, bf] = 1
        if sels[r] is not None:
            ft[r, bf[sels[r](mid)]] = 2
    return ft


@pytest.mark.parametrize("traction", [False, True])
@pytest.mark.parametrize("data", ["synthetic", "galerkin"])
@pytest.mark.parametrize("ns", [9, 12, 24, 40, 63])
def test_k4_disk(oracle_mod, ns, data, traction):
    from dolfinx_eqlb_amd.mesh import create_disk
    mesh = create_disk(ns, 2, shuffle_seed=11)
    ft, G, f, bv = disk_data(mesh, 4, traction, data)
    run_stress(oracle_mod, mesh, 4, ft, G, f, bv)


@pytest.mark.parametrize("traction", [False, True])
@pytest.mark.parametrize("data", ["synthetic", "galerkin"])
@pytest.mark.parametrize("ns", [40, 63])
def test_k3_disk(oracle_mod, ns, data, traction):
    from dolfinx_eqlb_amd.mesh import create_disk
    mesh = create_disk(ns, 3, shuffle_seed=12)
    ft, G, f, bv = disk_data(mesh, 3, traction, data)
    run_stress(oracle_mod, mesh, 3, ft, G, f, bv)


@pytest.mark.parametrize("k", [3, 4])
def test_delaunay_all_bins(oracle_mod, k):
    mesh = delaunay_mesh(700, seed=5)
    val = np.diff(mesh.node_cells_offsets)
    assert val.max() >= 9 and (val <= 8).sum() > 0  # small and large bins in one call
    ft = flux_types(mesh, [lambda m: m[:, 0] < -0.3, lambda m: m[:, 1] > 0.2])
    G, f, bv = gk.solve_elasticity(mesh, k, ft, seed=7 * k)
    run_stress(oracle_mod, mesh, k, ft, G, f, bv)


def half_annulus(m):
    """Centre node 0 on the straight boundary with a fan of m cells, ring 1 (radius 1) and ring 2 (radius 2) of
    m + 1 nodes each over the upper half plane; every node has at least two cells."""
    from dolfinx_eqlb_amd.mesh import create_mesh
    j = np.arange(m + 1)
    th = np.linspace(0.0, np.pi, m + 1) + 0.2 * np.pi / m * np.sin(2.3 * j) * (j % m > 0)  # perturbed, ends fixed
    a = 1 + np.arange(m + 1)
    b = 2 + m + np.arange(m + 1)
    x = np.concatenate([[[0.0, 0.0]], np.stack([np.cos(th), np.sin(th)], 1),
                        2.0 * np.stack([np.cos(th), np.sin(th)], 1)])
    cells = [[0, a[i], a[i + 1]] for i in range(m)]
    for i in range(m - 1):
        cells += [[a[i], b[i], a[i + 1]], [a[i + 1], b[i], b[i + 1]]]
    cells += [[a[m - 1], b[m - 1], b[m]], [a[m - 1], b[m], a[m]]]
    return create_mesh(x, np.array(cells, dtype=np.int32))


@pytest.mark.parametrize("k,m", [(4, 9), (4, 20), (4, 40), (3, 33), (3, 63)])
@pytest.mark.parametrize("layout", ["row0", "both_meanvalue", "both_one_side"])
def test_large_boundary_patch(oracle_mod, k, m, layout):
    """Boundary patch of m cells around the centre: tractions on the straight side in row 0 only, on both sides
    of the centre in both rows (mean-value multiplier), or on one side in both rows (no multiplier)."""
    mesh = half_annulus(m)
    straight = lambda p: np.abs(p[:, 1]) < 1e-12  # noqa: E731
    if layout == "row0":
        sels = [straight, None]
    elif layout == "both_meanvalue":
        sels = [straight, straight]
    else:
        sels = [lambda p: straight(p) & (p[:, 0] > 0.0)] * 2
    ft = flux_types(mesh, sels)
    G, f, bv = gk.solve_elasticity(mesh, k, ft, seed=3 * m + k)
    run_stress(oracle_mod, mesh, k, ft, G, f, bv)


@pytest.mark.parametrize("k,m", [(4, 10), (4, 30), (3, 40)])
@pytest.mark.parametrize("order", [0, 1])
def test_grouped_large_patches(oracle_mod, k, m, order):
    from synthetic import facet_types, make_compatible_stress_data
    mesh = big_double_fan_mesh(m, order)
    val = np.diff(mesh.node_cells_offsets)
    assert val.max() == m + 3 and (val == 2).sum() >= 4
    ft = np.repeat(facet_types(mesh, lambda p: np.ones(len(p), dtype=bool)), 2, axis=0)
    G, f = make_compatible_stress_data(mesh, k, ft)
    run_stress(oracle_mod, mesh, k, ft, G, f)


def test_public_interface_k4_delaunay_korn(oracle_mod):
    """FluxEqlbSE (stress + Korn constants) at RT_4 on a Delaunay mesh: predicates, oracle, Korn constants."""
    from dolfinx_eqlb_amd.eqlb import check_eqlb_conditions as chk
    from dolfinx_eqlb_amd.eqlb.FluxEqlbSE import FluxEqlbSE, fluxbc
    k = 4
    mesh = delaunay_mesh(500, seed=9)
    assert np.diff(mesh.node_cells_offsets).max() >= 9
    bf = mesh.boundary_facets()
    mid = mesh.x[mesh.facet_nodes[bf]].mean(axis=1)[:, :2]
    trac = bf[mid[:, 1] > 0.1]
    disp = bf[~(mid[:, 1] > 0.1)]
    ft = np.zeros((2, mesh.nfacets), dtype=np.int8)
    ft[:, disp] = 1
    ft[:, trac] = 2
    G, f, bv = gk.solve_elasticity(mesh, k, ft, seed=77, traction=lambda r, x, y: 0.0 * x)
    eq = FluxEqlbSE(k, mesh, [f[0], f[1]], [G[0], G[1]], True, True)
    eq.set_boundary_conditions([disp, disp], [[fluxbc(0, trac, eq.V_flux)], [fluxbc(0, trac, eq.V_flux)]])
    assert np.array_equal(eq.facet_type, ft)
    eq.equilibrate_fluxes()
    x = eq.list_flux
    scale = np.abs(x).max()
    for r in range(2):
        res, nrm = chk.divergence_residual(mesh, k, x[r], G[r], f[r])
        assert res <= 1e-10 * max(nrm, scale)
        assert chk.jump_residual(mesh, k, x[r], G[r]) <= 1e-9 * scale
        assert chk.boundary_flux_residual(mesh, k, x[r], G[r], trac) <= 1e-10 * max(1.0, scale)
    assert np.abs(asym_moments(mesh, k, x)[1]).max() < 1e-11 * max(1.0, scale)
    assert chk.check_weak_symmetry_condition(mesh, k, x)
    ref = oracle_mod.se_reconstruct(mesh, k, ft, G, f, stress=True)
    assert np.abs(x - ref).max() <= 1e-10 * np.abs(ref).max()
    assert np.allclose(eq.get_korn_constants(), np.sqrt(oracle_mod.se_korn(mesh, ft)), rtol=1e-12)
