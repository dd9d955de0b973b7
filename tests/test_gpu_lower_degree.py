"""Projected data of degree d < k-1 (flux_dg, rhs_dg in DG_d; se/reconstruction.hpp:363-373) equilibrated on the
device without embedding into DG_{k-1}: SE, stress and EV against the oracles, through the C ABI, the pybind module
and the mirror classes.  The EV oracle builds DG_{k-1} only: it is fed embed_dg(data), the same minimisation problem
(DG_d is a subspace of DG_{k-1}).  Tolerances as tests/test_gpu_parity.py (1e-11 of the largest DOF; k = 4 and
stress 1e-10)."""

import numpy as np
import pytest

import tile_classes as tcl
from cases import BCS
from dolfinx_eqlb_amd.eqlb import check_eqlb_conditions as chk
from dolfinx_eqlb_amd.eqlb.conforming import conforming_dofmap, conforming_to_broken
from dolfinx_eqlb_amd.lsolver import embed_dg
from dolfinx_eqlb_amd.mesh import create_unit_square
from synthetic import boundary_dofs_from_field, facet_types, make_compatible_data

pytestmark = pytest.mark.gpu

NEW_PAIRS = [(2, 0), (3, 1), (3, 0), (4, 2), (4, 1), (4, 0)]
IDS = [f"k{k}d{d}" for k, d in NEW_PAIRS]


def _tol(k, stress=False):
    return 1e-10 if (k == 4 or stress) else 1e-11


def _close(x, ref, tol):
    return np.abs(x - ref).max() <= tol * np.abs(ref).max()


@pytest.fixture(scope="module")
def cpp():
    from dolfinx_eqlb_amd import cpp as c
    assert c.device_count() >= 1, "GPU tests need a HIP device"
    return c


def _embed(G, f, ncells, d, k):
    """DG_d -> DG_{k-1} of stacked [nrhs, ...] data."""
    Ge = np.stack([embed_dg(g, ncells, d, k - 1, bs=2) for g in G])
    fe = np.stack([embed_dg(r, ncells, d, k - 1) for r in f])
    return Ge, fe


def _w(x, y):
    return 1.0 + 0.5 * x - 0.3 * y, -0.7 + 0.2 * x + 0.4 * y


def _se_case(k, d, bc, n=6, seed=20241003):
    mesh = create_unit_square(n, shuffle_seed=8, perturb=0.25)
    if bc == "inhomogeneous":
        ft = facet_types(mesh, BCS["neumann_lt"])
        G, f = make_compatible_data(mesh, k, ft, degree_dg=d, neumann_flux=_w, seed=seed)
        bv = boundary_dofs_from_field(mesh, k, ft[0], _w)[None]
    else:
        ft = facet_types(mesh, BCS[bc])
        G, f = make_compatible_data(mesh, k, ft, degree_dg=d, seed=seed)
        bv = None
    return mesh, ft, G[None], f[None], bv


# ------------------------------------------------------------------------------------------------------------- SE
@pytest.mark.parametrize("bc", ["dirichlet", "neumann_lt", "inhomogeneous"])
@pytest.mark.parametrize("k,d", NEW_PAIRS, ids=IDS)
def test_se_matches_oracle(cpp, oracle_mod, k, d, bc):
    """Every launch family of the pair against the oracle at degree d; the same call on embed_dg(data) at
    d = k-1 agrees to 1e-12 (k = 4: 1e-11)."""
    mesh, ft, G, f, bv = _se_case(k, d, bc)
    ref = oracle_mod.se_reconstruct(mesh, k, ft, G, f, boundary_values=bv, degree_dg=d)
    dm = cpp.DeviceMesh(mesh)
    variants = [dict(), dict(scatter=0), dict(scatter=2), dict(scatter=0, fused=0), dict(solver=0, scatter=0)] \
        if k <= 3 else [dict(solver=0), dict(solver=1), dict(solver=1, scatter=1)]
    out = []
    for opts in variants:
        eq = cpp.SemiExplicitEquilibrator(dm, k, 1, degree_dg=d)
        for key, v in opts.items():
            eq.set_option(key, v)
        eq.set_boundary(ft, boundary_values=bv)
        x = eq.equilibrate_host(G, f)
        assert _close(x, ref, _tol(k)), opts
        out.append(x)
    Ge, fe = _embed(G, f, mesh.ncells, d, k)
    eqe = cpp.SemiExplicitEquilibrator(dm, k, 1)
    eqe.set_boundary(ft, boundary_values=bv)
    # (RT_4: the two data layouts round apart by up to 1.1e-12 - its oracle bound is 1e-10, ten times that of k <= 3)
    assert np.abs(eqe.equilibrate_host(Ge, fe) - out[0]).max() <= (1e-11 if k == 4 else 1e-12) * np.abs(out[0]).max()
    res, nrm = chk.divergence_residual(mesh, k, out[0][0], G[0], f[0], degree_dg=d)
    assert res <= 1e-10 * nrm
    assert chk.check_jump_condition(mesh, k, out[0][0], G[0], degree_dg=d, atol=1e-9)


@pytest.mark.parametrize("k,d", NEW_PAIRS, ids=IDS)
def test_se_multirhs_mask_and_device_stream(cpp, oracle_mod, k, d):
    """R = 3 right-hand sides with different boundary conditions, a node mask, device memory on a non-blocking
    stream."""
    import torch
    mesh = create_unit_square(7, shuffle_seed=3, perturb=0.2)
    names = ["neumann_lt", "dirichlet", "neumann_bottom"]
    ft = np.stack([facet_types(mesh, BCS[n])[0] for n in names])
    data = [make_compatible_data(mesh, k, ft[i:i + 1], degree_dg=d, seed=11 + i) for i in range(3)]
    G = np.stack([a[0] for a in data])
    f = np.stack([a[1] for a in data])
    mask = (mesh.x[:, 0] < 0.5).astype(np.uint8)
    ref = np.zeros((3, mesh.ncells * k * (k + 2)))
    for node in np.nonzero(mask)[0]:
        oracle_mod.se_reconstruct(mesh, k, ft, G, f, degree_dg=d, flux_hdiv=ref, node_range=(int(node), int(node) + 1))
    dm = cpp.DeviceMesh(mesh)
    eq = cpp.SemiExplicitEquilibrator(dm, k, 3, degree_dg=d)
    eq.set_boundary(ft, node_mask=mask)
    x = eq.equilibrate_host(G, f)
    assert _close(x, ref, _tol(k))
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    g_dev = torch.from_numpy(G).to(dev)
    f_dev = torch.from_numpy(f).to(dev)
    x_dev = torch.zeros(x.shape, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        eq.equilibrate_device(g_dev.data_ptr(), f_dev.data_ptr(), x_dev.data_ptr(), stream=s.cuda_stream)
    eq.check_status(s.cuda_stream)
    assert np.array_equal(x_dev.cpu().numpy(), x)


def test_create_accepts_every_pair_and_keeps_the_refusals(cpp):
    dm = cpp.DeviceMesh(create_unit_square(2))
    for k in range(1, 5):
        for d in range(k):
            cpp.SemiExplicitEquilibrator(dm, k, 1, degree_dg=d).close()
            cpp.ConstrainedMinEquilibrator(dm, k, 1, degree_dg=d).close()
    for k, d in [(2, 2), (3, -1), (1, 1)]:
        with pytest.raises(RuntimeError, match="Wrong polynomial degree"):
            cpp.SemiExplicitEquilibrator(dm, k, 1, degree_dg=d)
    with pytest.raises(RuntimeError, match="not in this build"):
        cpp.SemiExplicitEquilibrator(dm, 5, 1, degree_dg=3)


# --------------------------------------------------------------------------------------------------------- stress
def _stress_data(mesh, k, d, ft):
    """Galerkin elasticity in P_{d+1}: G (rows of -sigma(u_h), symmetric) and f in DG_d, homogeneous tractions."""
    import galerkin as gk
    G, f, _ = gk.solve_elasticity(mesh, d + 1, ft, seed=3, traction=lambda r, x, y: 0.0 * x)
    return G, f


def _asym_total(mesh, k, d, x, G):
    """Assembled (sigma_01 - sigma_10, hat_a) of the equilibrated stress sigma = x + G."""
    from dolfinx_eqlb_amd.elmtlib.lagrange import Lagrange
    from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
    from test_oracle_stress import asym_moments
    J, detJ, K = chk.cell_geometry(mesh)
    qp, qw = make_quadrature_triangle(k + 2)
    psi = Lagrange(d).tabulate(qp)[0]
    hv = Lagrange(1).tabulate(qp)[0]
    g = np.asarray(G).reshape(2, mesh.ncells, -1, 2)
    a = np.einsum("qi,ci->cq", psi, g[0, ..., 1] - g[1, ..., 0])
    loc = np.einsum("cq,cq,qn->cn", qw[None] * np.abs(detJ)[:, None], a, hv)
    L = np.zeros(mesh.nnodes)
    np.add.at(L, mesh.cell_nodes.ravel(), loc.ravel())
    return asym_moments(mesh, k, x)[1] + L


# (RT_2 / DG_0 with tractions - grouped boundary patches - is left out: P1 Galerkin stresses do not satisfy the moment
# balance those groups need)
STRESS = [(2, 0, "dirichlet"), (3, 1, "dirichlet"), (3, 1, "traction"), (3, 0, "dirichlet"),
          (4, 2, "dirichlet"), (4, 1, "traction")]


@pytest.mark.parametrize("k,d,bc", STRESS, ids=[f"k{k}d{d}-{b}" for k, d, b in STRESS])
def test_stress_matches_oracle(cpp, oracle_mod, k, d, bc):
    """Stress rows with weak symmetry; RT_2 / DG_0 runs the slot path and the weak-symmetry kernel of the stress
    flux-BC route.  Korn constants against the oracle."""
    import galerkin as gk
    mesh = create_unit_square(5, shuffle_seed=6, perturb=0.2)
    layout = [[True, False], [True, False]] if bc == "traction" else []  # (row 0: tractions on x = 0, y = 0)
    ft = gk.elasticity_facet_types(mesh, layout)
    G, f = _stress_data(mesh, k, d, ft)
    ref = oracle_mod.se_reconstruct(mesh, k, ft, G, f, degree_dg=d, stress=True)
    eq = cpp.SemiExplicitEquilibrator(cpp.DeviceMesh(mesh), k, 2, degree_dg=d, reconstruct_stress=True,
                                      estimate_korn=True)
    eq.set_boundary(ft)
    x, korn = eq.equilibrate_host_with_kornconst(G, f)
    # (RT_4 with tractions on the Galerkin stress: 1.13e-10 measured; the same call at DG_3 on embed_dg(data) - the
    # existing RT_4 stress path - agrees with this result to 1e-11 below, so the gap to the oracle is RT_4 rounding)
    assert _close(x, ref, 2e-10 if k == 4 else _tol(k, True)), np.abs(x - ref).max() / np.abs(ref).max()
    Ge, fe = _embed(G, f, mesh.ncells, d, k)
    eqe = cpp.SemiExplicitEquilibrator(cpp.DeviceMesh(mesh), k, 2, reconstruct_stress=True)
    eqe.set_boundary(ft)
    xe = eqe.equilibrate_host(Ge, fe)
    assert np.abs(xe - x).max() <= (1e-11 if k == 4 else 1e-12) * np.abs(x).max(), np.abs(xe - x).max() / np.abs(x).max()
    if d >= 1:
        # (P1 Galerkin data - d = 0 - do not satisfy the moment balance against x hat_a, which is not in P1: the oracle
        # leaves the same asymmetry there, with native and with embedded data alike; the comparison above pins it)
        assert np.abs(_asym_total(mesh, k, d, x, G)).max() < 1e-11
    kref = oracle_mod.se_korn(mesh, ft)
    assert np.abs(korn - kref).max() <= 1e-12 * np.abs(kref).max()
    assert np.array_equal(eq.equilibrate_host(G, f), x)


# ------------------------------------------------------------------------------------------------------------- EV
# (k = 4: the EV patch problems run on the slot path only)
EV = [(k, d, sc) for k, d in NEW_PAIRS for sc in ((0, 2) if k <= 3 else (0,))]


@pytest.mark.parametrize("k,d,scatter", EV, ids=[f"k{k}d{d}-sc{sc}" for k, d, sc in EV])
def test_ev_matches_embedded_oracle(cpp, oracle_mod, k, d, scatter):
    mesh, ft, G, f, _ = _se_case(k, d, "neumann_lt")
    cd, nd = conforming_dofmap(mesh, k)
    Ge, fe = _embed(G, f, mesh.ncells, d, k)
    ref = oracle_mod.ev_reconstruct(mesh, k, ft, Ge, fe, cd, nd)
    eq = cpp.ConstrainedMinEquilibrator(cpp.DeviceMesh(mesh), k, 1, degree_dg=d)
    eq.set_option("scatter", scatter)
    eq.set_boundary(ft)
    x = eq.equilibrate_host(G, f)
    assert _close(x, ref, _tol(k))
    eq.set_option("output", 1)
    xb = eq.equilibrate_host(G, f)[0]
    assert _close(xb, conforming_to_broken(mesh, k, ref[0]), _tol(k))


# ------------------------------------------------------------------------------------------- the reference's matrix
def _galerkin_poisson(mesh, k, seed=0):
    """P_{k-1} Galerkin solution of -div grad u = f_h, u = 0 on the boundary, with f_h a DG_{k-2} field: the projected
    flux G = -grad u_h and the right-hand side f_h in DG_{k-2} (test_fluxeqlb_conditions.py:62-67)."""
    import galerkin as gk
    from dolfinx_eqlb_amd.elmtlib.lagrange import Lagrange
    kp, d = k - 1, k - 2
    f = 1.0 + np.random.default_rng(seed).random(mesh.ncells * Lagrange(d).ndofs)
    u, cd = gk.solve_poisson(mesh, kp, None, f_dg=f)
    return gk.discrete_flux(mesh, kp, u, cd), f


def _meshes():
    from test_gpu_unstructured import delaunay_mesh
    return {"crossed2": create_unit_square(2), "delaunay": delaunay_mesh(150, seed=4)}


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("mesh_name", ["crossed2", "delaunay"])
def test_reference_matrix_through_the_mirrors(cpp, oracle_mod, mesh_name, k):
    """P_{k-1} primal, projected flux and RHS in DG_{k-2}, through FluxEqlbSE / FluxEqlbEV (the pybind module's
    reconstruct_fluxes_semiexplt / reconstruct_fluxes_minimisation) with the data as they are."""
    from dolfinx_eqlb_amd.eqlb.FluxEqlbEV import FluxEqlbEV
    from dolfinx_eqlb_amd.eqlb.FluxEqlbSE import FluxEqlbSE
    mesh = _meshes()[mesh_name]
    d = k - 2
    G, f = _galerkin_poisson(mesh, k)
    ft = facet_types(mesh, None)
    bf = mesh.boundary_facets()
    se = FluxEqlbSE(k, mesh, [f], [G])
    assert se.degree_dg == d
    se.set_boundary_conditions([bf], [[]])
    se.equilibrate_fluxes()
    x, proj = se.get_reconstructed_fluxes(0)
    assert np.array_equal(proj, G)  # the caller's projected flux, not an embedded copy
    ref = oracle_mod.se_reconstruct(mesh, k, ft, G[None], f[None], degree_dg=d)[0]
    assert _close(x, ref, _tol(k))
    res, nrm = chk.divergence_residual(mesh, k, x, G, f, degree_dg=d)
    assert res <= 1e-10 * nrm
    assert chk.check_divergence_condition(mesh, k, x, G, f, degree_dg=d)
    assert chk.check_jump_condition(mesh, k, x, G, degree_dg=d, atol=1e-9)
    ev = FluxEqlbEV(k, mesh, [f], [G])
    ev.set_boundary_conditions([bf], [[]])
    ev.equilibrate_fluxes()
    cd, nd = conforming_dofmap(mesh, k)
    Ge, fe = _embed(G[None], f[None], mesh.ncells, d, k)
    refe = oracle_mod.ev_reconstruct(mesh, k, ft, Ge, fe, cd, nd)[0]
    xe = ev.get_reconstructed_fluxes(0)
    assert _close(xe, refe, _tol(k))
    xb = conforming_to_broken(mesh, k, xe)
    zG = np.zeros_like(G)
    res, nrm = chk.divergence_residual(mesh, k, xb, zG, f, degree_dg=d)
    assert res <= 1e-10 * nrm
    assert chk.check_jump_condition(mesh, k, xb, zG, degree_dg=d, atol=1e-9)


# --------------------------------------------------------------------------------------------- tiled instances
def _tile_cases():
    from test_gpu_tile_dispatch import _crossed_masks, _fan_masks, _valence_masks
    return ([("crossed", i, m) for i, m in enumerate(_crossed_masks())]
            + [("valence", i, m) for i, m in enumerate(_valence_masks())]
            + [("fans", i, m) for i, m in enumerate(_fan_masks())])


TILE_CASES = _tile_cases()


@pytest.mark.parametrize("k,d", [(2, 0), (3, 1)], ids=["k2d0", "k3d1"])
@pytest.mark.parametrize("mesh_name,i,counts", TILE_CASES, ids=[f"{n}{i}" for n, i, _ in TILE_CASES])
def test_tiled_instances_at_lower_degree(cpp, oracle_mod, mesh_name, i, counts, k, d):
    """Single-tile meshes and masks whose class counts sit on the wave-block boundaries: every body instance of the
    flux sweep (full, interior, generic) runs at the new DEG, every cell against the oracle, bitwise
    repeatable, and the wave-blocks are the predicted ones."""
    from test_gpu_tile_dispatch import _oracle_se, class_mask, mesh_of
    mesh = mesh_of(mesh_name)
    mask = class_mask(mesh, counts, seed=i)
    ft = facet_types(mesh, None)
    G, f = make_compatible_data(mesh, k, ft, degree_dg=d, seed=17)
    G, f = G[None], f[None]
    eq = cpp.SemiExplicitEquilibrator(cpp.DeviceMesh(mesh), k, 1, degree_dg=d)
    eq.set_option("scatter", 2)
    eq.set_boundary(ft, node_mask=mask)
    x1 = eq.equilibrate_host(G, f)
    x2 = eq.equilibrate_host(G, f)
    assert np.array_equal(x1, x2)
    ref = np.zeros_like(x1)
    for node in np.nonzero(mask)[0]:
        oracle_mod.se_reconstruct(mesh, k, ft, G, f, degree_dg=d, flux_hdiv=ref, node_range=(int(node), int(node) + 1))
    assert np.abs(x1 - ref).max() <= 1e-11 * max(np.abs(ref).max(), 1e-300)
    assert eq.tiling_blocks() == tcl.predict(mesh, k, mask)


def test_tiled_instance_classes_are_all_reached():
    """The cases above run every body instance of the flux sweep (host-side count): full, interior (RT_2 only) and
    generic.  (The NFIX instances belong to the fused RT_2 stress launch, which DG_0 data do not take.)"""
    from test_gpu_tile_dispatch import class_mask, mesh_of
    for k, kinds in ((2, ("full", "interior", "generic")), (3, ("full", "generic"))):
        seen = dict.fromkeys(kinds, 0)
        for name, i, counts in TILE_CASES:
            mesh = mesh_of(name)
            tb = tcl.predict(mesh, k, class_mask(mesh, counts, seed=i))
            for kind in kinds:
                seen[kind] += sum(tb[kind])
        assert all(v > 0 for v in seen.values()), (k, seen)


# ------------------------------------------------------------------------------------------------- 1M triangles
def test_one_million_triangles_rt2_dg0(cpp, oracle_mod):
    from dolfinx_eqlb_amd.mesh import create_unit_square as cus
    k, d = 2, 0
    mesh = cus(500, shuffle_seed=1234)
    ft = facet_types(mesh)
    G, f = make_compatible_data(mesh, k, ft, degree_dg=d)
    eq = cpp.SemiExplicitEquilibrator(cpp.DeviceMesh(mesh), k, 1, degree_dg=d)
    eq.set_boundary(ft)
    x = eq.equilibrate_host(G[None], f[None])
    assert np.array_equal(x, eq.equilibrate_host(G[None], f[None]))
    res, nrm = chk.divergence_residual(mesh, k, x[0], G, f, degree_dg=d)
    assert res <= 1e-10 * nrm
    rng = np.random.default_rng(0)
    mask = np.zeros(mesh.nnodes, dtype=np.uint8)
    mask[rng.choice(mesh.nnodes, 2000, replace=False)] = 1
    eqm = cpp.SemiExplicitEquilibrator(cpp.DeviceMesh(mesh), k, 1, degree_dg=d)
    eqm.set_boundary(ft, node_mask=mask)
    xm = eqm.equilibrate_host(G[None], f[None])
    ref = np.zeros_like(xm)
    for node in np.nonzero(mask)[0]:
        oracle_mod.se_reconstruct(mesh, k, ft, G[None], f[None], degree_dg=d, flux_hdiv=ref,
                                  node_range=(int(node), int(node) + 1))
    assert np.abs(xm - ref).max() <= 1e-11 * np.abs(ref).max()
