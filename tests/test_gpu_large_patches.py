"""Vertex patches of more than 63 cells on the device (option "large_patches": one workgroup per patch,
eqlb_se_large.hip) against the oracle: polar disks whose hub has 64 ... 257 cells, half annuli whose hub lies on the
boundary, SE and EV, every scatter mode, lower data degrees, several right-hand sides, node masks, device memory on
a caller's stream, the pybind module and the mirrors.

Bound of every device-vs-oracle comparison, relative to max |oracle|: max(1e-11, 10 x the discrepancy recorded for
the case in tests/test_large_patches_oracle.py) - 1e-11 is what the high-valence tests of the one-wave path use, the
record is what two elimination orders on such a fan differ by on the CPU already (RT_1 ... RT_3: oracle vs independent
minimiser; RT_4: oracle vs the numpy statement of the device formulation, see that file), the factor 10 allows for
the device's third order.  Every cell of the mesh is compared."""

import functools

import numpy as np
import pytest

from dolfinx_eqlb_amd.eqlb import check_eqlb_conditions as chk
from dolfinx_eqlb_amd.eqlb.conforming import broken_to_conforming, conforming_dofmap, conforming_to_broken
from dolfinx_eqlb_amd.lsolver import embed_dg
from dolfinx_eqlb_amd.mesh import create_disk, create_mesh, create_unit_square
from synthetic import boundary_dofs_from_field, facet_types, make_compatible_data
from test_large_patches_oracle import (STRAIGHT_LAYOUTS, annulus_case, disk_case, half_annulus, hub_discrepancy,
                                       hub_node)

pytestmark = pytest.mark.gpu


def bound(kind, n, nr, k):
    return max(1e-11, 10.0 * hub_discrepancy(kind, n, nr, k))


@pytest.fixture(scope="module")
def cpp():
    from dolfinx_eqlb_amd import cpp as c
    assert c.device_count() >= 1, "GPU tests need a HIP device"
    return c


@functools.lru_cache(maxsize=None)
def _disk(ns, nr, k, d=None):
    return disk_case(ns, nr, k, degree_dg=d)


_REF = {}


def _se_ref(oracle_mod, key, mesh, k, ft, G, f, **kw):
    if key not in _REF:
        _REF[key] = oracle_mod.se_reconstruct(mesh, k, ft, G, f, **kw)
    return _REF[key]


def _rel(x, ref):
    return np.abs(x - ref).max() / np.abs(ref).max()


def _check(name, x, ref, tol):
    err = _rel(x, ref)
    print(f"{name}: device vs oracle {err:.2e} (bound {tol:.1e})")
    assert np.isfinite(x).all() and err <= tol, (name, err, tol)


def _predicates(mesh, k, x, G, f, d=None):
    res, nrm = chk.divergence_residual(mesh, k, x, G, f, degree_dg=d)
    assert res <= 1e-10 * nrm
    assert chk.check_jump_condition(mesh, k, x, G, degree_dg=d, atol=1e-9)


def _se_handle(cpp, mesh, k, nrhs=1, d=None, scatter=None, accumulate=1, **opts):
    eq = cpp.SemiExplicitEquilibrator(cpp.DeviceMesh(mesh), k, nrhs, degree_dg=d)
    if scatter is not None:
        eq.set_option("scatter", scatter)
    eq.set_option("accumulate", accumulate)
    for key, v in opts.items():
        eq.set_option(key, v)
    eq.set_option("large_patches", 1)
    return eq


# ---------------------------------------------------------------------------------------------------------- SE, disks
# (the tiled scatter exists for k <= 3; RT_4 runs the slot path, chosen or automatic)
SE_CASES = [(k, ns, sc, acc) for k in (1, 2, 3, 4) for ns in (64, 65, 70, 100, 128, 257)
            for sc in ((0, 2, None) if k <= 3 else (0, None)) for acc in (0, 1)]


@pytest.mark.parametrize("k,ns,scatter,accumulate", SE_CASES,
                         ids=[f"k{k}-ns{ns}-sc{'auto' if sc is None else sc}-acc{a}" for k, ns, sc, a in SE_CASES])
def test_se_disk(cpp, oracle_mod, k, ns, scatter, accumulate):
    """Hub of ns cells, two rings (the small ring patches and the hub share cells), flux BC on the upper half of the
    rim.  accumulate = 0 has to overwrite a pre-filled vector, accumulate = 1 to add to it."""
    mesh, ft, G, f = _disk(ns, 2, k)
    ref = _se_ref(oracle_mod, ("disk", ns, k), mesh, k, ft, G, f)
    eq = _se_handle(cpp, mesh, k, scatter=scatter, accumulate=accumulate)
    eq.set_boundary(ft)
    assert eq.large_patch_info() == (1, ns)
    pre = np.full(ref.shape, 0.375)
    x = eq.equilibrate_host(G, f, pre.copy())
    if accumulate:
        x = x - pre
    _check(f"disk {ns} k={k}", x, ref, bound("disk", ns, 2, k))
    _predicates(mesh, k, x[0], G[0], f[0])
    assert np.array_equal(eq.equilibrate_host(G, f, pre.copy()) - (pre if accumulate else 0.0), x)  # determinism


# ---------------------------------------------------------------------------------------------------- boundary fans
def _w(k):
    if k == 1:
        return lambda x, y: (0 * x + 0.8, 0 * x - 0.6)
    return lambda x, y: (1.0 + 0.5 * x - 0.3 * y, -0.7 + 0.2 * x + 0.4 * y)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("m", [64, 100])
@pytest.mark.parametrize("layout", ["dirichlet", "flux_one_side", "flux_both_sides", "inhomogeneous"])
def test_se_boundary_fan(cpp, oracle_mod, k, m, layout):
    """Hub on the straight side of a half annulus: open chain, flux BC on one or on both end facets of the fan,
    prescribed (inhomogeneous) normal fluxes."""
    bv = None
    if layout == "inhomogeneous":
        mesh = half_annulus(m)
        ft = facet_types(mesh, STRAIGHT_LAYOUTS["flux_both_sides"])
        G, f = make_compatible_data(mesh, k, ft, neumann_flux=_w(k))
        G, f = G[None], f[None]
        bv = boundary_dofs_from_field(mesh, k, ft[0], _w(k))[None]
        assert np.abs(bv).max() > 1e-3
    else:
        mesh, ft, G, f = annulus_case(m, k, layout)
    ref = oracle_mod.se_reconstruct(mesh, k, ft, G, f, boundary_values=bv)
    for scatter in ((0, None) if k <= 3 else (0,)):
        eq = _se_handle(cpp, mesh, k, scatter=scatter)
        eq.set_boundary(ft, boundary_values=bv)
        assert eq.large_patch_info() == (1, m)
        x = eq.equilibrate_host(G, f)
        _check(f"annulus {m} {layout} k={k}", x, ref, bound("annulus", m, 2, k))
        _predicates(mesh, k, x[0], G[0], f[0])
        assert np.array_equal(eq.equilibrate_host(G, f), x)


# ------------------------------------------------------------------------------------------------------------ EV
def _ev_run(cpp, oracle_mod, name, mesh, ft, G, f, k, tol, nlarge):
    cd, nd = conforming_dofmap(mesh, k)
    ref = oracle_mod.ev_reconstruct(mesh, k, ft, G, f, cd, nd)
    for scatter in (0, 2, None):
        eq = cpp.ConstrainedMinEquilibrator(cpp.DeviceMesh(mesh), k, 1)
        if scatter is not None:
            eq.set_option("scatter", scatter)
        eq.set_option("large_patches", 1)
        eq.set_boundary(ft)
        assert eq.large_patch_info() == nlarge
        x = eq.equilibrate_host(G, f)
        err = np.abs(x - ref).max() / np.abs(ref).max()
        print(f"{name} EV k={k} scatter={scatter}: {err:.2e} (bound {tol:.1e})")
        assert np.isfinite(x).all() and err <= tol
        assert np.array_equal(eq.equilibrate_host(G, f), x)
        eq.set_option("output", 1)  # broken hierarchic layout
        xb = eq.equilibrate_host(G, f)[0]
        refb = conforming_to_broken(mesh, k, ref[0])
        assert np.abs(xb - refb).max() <= tol * np.abs(refb).max()
        # (the EV result is the whole flux, not a corrector of G: predicates with G = 0)
        res, nrm = chk.divergence_residual(mesh, k, xb, np.zeros_like(G[0]), f[0])
        assert res <= 1e-10 * max(nrm, 1.0)
        assert chk.check_jump_condition(mesh, k, xb, np.zeros_like(G[0]), atol=1e-9)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("ns", [70, 128])
def test_ev_disk(cpp, oracle_mod, k, ns):
    mesh, ft, G, f = _disk(ns, 2, k)
    _ev_run(cpp, oracle_mod, f"disk {ns}", mesh, ft, G, f, k, bound("disk", ns, 2, k), (1, ns))


@pytest.mark.parametrize("k", [1, 2, 3])
def test_ev_boundary_fan(cpp, oracle_mod, k):
    mesh, ft, G, f = annulus_case(100, k, "flux_one_side")
    _ev_run(cpp, oracle_mod, "annulus 100", mesh, ft, G, f, k, bound("annulus", 100, 2, k), (1, 100))


# --------------------------------------------------------------------------------------------- lower data degrees
LOW = [(2, 0), (3, 1), (3, 0), (4, 2), (4, 1), (4, 0)]


@pytest.mark.parametrize("k,d", LOW, ids=[f"k{k}d{d}" for k, d in LOW])
def test_lower_data_degree(cpp, oracle_mod, k, d):
    mesh, ft, G, f = _disk(70, 2, k, d)
    tol = bound("disk", 70, 2, k)
    ref = oracle_mod.se_reconstruct(mesh, k, ft, G, f, degree_dg=d)
    for scatter in ((0, None) if k <= 3 else (0,)):
        eq = _se_handle(cpp, mesh, k, d=d, scatter=scatter)
        eq.set_boundary(ft)
        assert eq.large_patch_info() == (1, 70)
        x = eq.equilibrate_host(G, f)
        _check(f"disk 70 k={k} d={d}", x, ref, tol)
        _predicates(mesh, k, x[0], G[0], f[0], d)
    if k <= 3:  # EV against the oracle on the embedded data (as tests/test_gpu_lower_degree.py)
        cd, nd = conforming_dofmap(mesh, k)
        Ge = np.stack([embed_dg(g, mesh.ncells, d, k - 1, bs=2) for g in G])
        fe = np.stack([embed_dg(r, mesh.ncells, d, k - 1) for r in f])
        refe = oracle_mod.ev_reconstruct(mesh, k, ft, Ge, fe, cd, nd)
        ev = cpp.ConstrainedMinEquilibrator(cpp.DeviceMesh(mesh), k, 1, degree_dg=d)
        ev.set_option("large_patches", 1)
        ev.set_boundary(ft)
        assert ev.large_patch_info() == (1, 70)
        xe = ev.equilibrate_host(G, f)
        assert np.abs(xe - refe).max() <= tol * np.abs(refe).max()


# ------------------------------------------------------------------------ several right-hand sides, masks, streams
def _three_rhs(k, ns=70):
    mesh = create_disk(ns, 2, shuffle_seed=7)
    sels = [lambda x: x[:, 1] > 0.0, None, lambda x: x[:, 0] < 0.2]
    ft = np.stack([facet_types(mesh, s)[0] for s in sels])
    data = [make_compatible_data(mesh, k, ft[i:i + 1], seed=11 + i) for i in range(3)]
    return mesh, ft, np.stack([a[0] for a in data]), np.stack([a[1] for a in data])


@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("multi_rhs", [0, 1])
def test_multi_rhs(cpp, oracle_mod, k, multi_rhs):
    """Three right-hand sides with different boundary types in one call."""
    mesh, ft, G, f = _three_rhs(k)
    ref = _se_ref(oracle_mod, ("rhs3", k), mesh, k, ft, G, f)
    for scatter in ((0, 2) if k <= 3 else (0,)):
        eq = _se_handle(cpp, mesh, k, nrhs=3, scatter=scatter, multi_rhs=multi_rhs)
        eq.set_boundary(ft)
        assert eq.large_patch_info() == (1, 70)
        x = eq.equilibrate_host(G, f)
        _check(f"3 rhs k={k} scatter={scatter}", x, ref, bound("disk", 70, 2, k))
        for r in range(3):
            _predicates(mesh, k, x[r], G[r], f[r])


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("scatter", [0, 2])
def test_node_mask(cpp, oracle_mod, k, scatter):
    mesh, ft, G, f = _disk(70, 2, k)
    hub = hub_node(mesh)
    tol = bound("disk", 70, 2, k)
    # the hub masked out: nothing is left for the large-patch kernel
    mask = np.ones(mesh.nnodes, dtype=np.uint8)
    mask[hub] = 0
    ref = np.zeros((1, mesh.ncells * k * (k + 2)))
    for node in np.nonzero(mask)[0]:
        oracle_mod.se_reconstruct(mesh, k, ft, G, f, flux_hdiv=ref, node_range=(int(node), int(node) + 1))
    eq = _se_handle(cpp, mesh, k, scatter=scatter)
    eq.set_boundary(ft, node_mask=mask)
    assert eq.large_patch_info() == (0, 0)
    _check(f"hub masked k={k}", eq.equilibrate_host(G, f), ref, tol)
    # only the hub
    only = (1 - mask).astype(np.uint8)
    ref = np.zeros((1, mesh.ncells * k * (k + 2)))
    oracle_mod.se_reconstruct(mesh, k, ft, G, f, flux_hdiv=ref, node_range=(hub, hub + 1))
    eq.set_boundary(ft, node_mask=only)
    assert eq.large_patch_info() == (1, 70)
    _check(f"hub only k={k}", eq.equilibrate_host(G, f), ref, tol)


def _two_fans():
    """Two disjoint disks in one mesh: hubs of 70 and of 100 cells."""
    a, b = create_disk(70, 2, shuffle_seed=3), create_disk(100, 2, shuffle_seed=4)
    xb = b.x[:, :2] + np.array([3.0, 0.0])
    x = np.concatenate([a.x[:, :2], xb])
    cells = np.concatenate([a.cell_nodes, b.cell_nodes + a.nnodes]).astype(np.int32)
    return create_mesh(x, cells)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_two_large_patches_in_one_call(cpp, oracle_mod, k):
    mesh = _two_fans()
    ft = facet_types(mesh, lambda x: x[:, 1] > 0.0)
    G, f = make_compatible_data(mesh, k, ft)
    G, f = G[None], f[None]
    ref = oracle_mod.se_reconstruct(mesh, k, ft, G, f)
    for scatter in (0, 2):
        eq = _se_handle(cpp, mesh, k, scatter=scatter)
        eq.set_boundary(ft)
        assert eq.large_patch_info() == (2, 100)
        x = eq.equilibrate_host(G, f)
        _check(f"two fans k={k}", x, ref, bound("disk", 100, 2, k))
        _predicates(mesh, k, x[0], G[0], f[0])
    # eqlb_se_export_patches holds the long fans (stride from eqlb_mesh_max_patch_cells)
    fans = eq.export_patches()
    assert sorted(fans["ncells"])[-2:] == [70, 100]
    orc = oracle_mod.build_patches(mesh, ft)
    for key in ("ncells", "cells", "fcts", "fcts_local", "inodes_local"):
        assert np.array_equal(np.asarray(fans[key]), np.asarray(orc[key])), key


@pytest.mark.parametrize("k,ev", [(2, False), (3, False), (2, True)])
def test_device_pointers_on_a_user_stream(cpp, oracle_mod, k, ev):
    """As tests/test_gpu_streams.py: inputs produced late on a non-blocking stream, the first call on a fresh handle
    included; equal to the host-memory call of a second handle."""
    import torch
    mesh, ft, G, f = _disk(70, 2, k)

    def handle():
        h = cpp.ConstrainedMinEquilibrator(cpp.DeviceMesh(mesh), k, 1) if ev \
            else cpp.SemiExplicitEquilibrator(cpp.DeviceMesh(mesh), k, 1)
        h.set_option("large_patches", 1)
        h.set_boundary(ft)
        assert h.large_patch_info() == (1, 70)
        return h

    ref = handle().equilibrate_host(G, f)
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    g_src, f_src = torch.from_numpy(G).to(dev), torch.from_numpy(f).to(dev)
    g_dev, f_dev = torch.full_like(g_src, float("nan")), torch.full_like(f_src, float("nan"))
    x_dev = torch.full((1, ref.shape[1]), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    h = handle()
    for call in range(2):
        with torch.cuda.stream(s):
            torch.cuda._sleep(40_000_000)
            g_dev.copy_(g_src)
            f_dev.copy_(f_src)
            x_dev.zero_()
            h.equilibrate_device(g_dev.data_ptr(), f_dev.data_ptr(), x_dev.data_ptr(), stream=s.cuda_stream)
            out = x_dev.clone()
            g_dev.fill_(float("nan"))
            f_dev.fill_(float("nan"))
            x_dev.fill_(float("nan"))
        h.check_status(s.cuda_stream)
        s.synchronize()
        assert np.array_equal(out.cpu().numpy(), ref), call


# ----------------------------------------------------------------------------------------------- nothing else moves
@pytest.mark.parametrize("k", [1, 2, 3])
def test_regular_mesh_is_untouched(cpp, k):
    """Without a large patch the option changes neither the launches (eqlb_se_tiling_blocks) nor one bit."""
    mesh = create_unit_square(24, shuffle_seed=2, perturb=0.15)
    ft = facet_types(mesh, lambda x: x[:, 0] < 0.3)
    G, f = make_compatible_data(mesh, k, ft)
    out = []
    for opt in (0, 1):
        for scatter in (None, 0):
            eq = cpp.SemiExplicitEquilibrator(cpp.DeviceMesh(mesh), k, 1)
            if scatter is not None:
                eq.set_option("scatter", scatter)
            eq.set_option("large_patches", opt)
            eq.set_boundary(ft)
            assert eq.large_patch_info() == (0, 0)
            out.append((eq.tiling_blocks(), eq.equilibrate_host(G[None], f[None])))
    for i in range(2):
        assert out[i][0] == out[2 + i][0]
        assert np.array_equal(out[i][1], out[2 + i][1])


# ------------------------------------------------------------------------------------------ module and mirrors
def _bd(c, mesh, k, ft, V, custom):
    nq = c.facet_quadrature(c.interpolation_quadrature_degree(k))[0].size
    bcs = [[c.FluxBC(V, [int(i) for i in np.nonzero(ft[0] == 2)[0]], 0, nq, [], [], [])]]
    prime = [[int(i) for i in np.nonzero(ft[0] == 1)[0]]]
    return c.BoundaryData(bcs, [c.Function(V)], V, custom, 2 * (k - 1), prime, False)


@pytest.mark.parametrize("k", [1, 2])
def test_option_through_the_pybind_module(oracle_mod, k):
    """BoundaryData.set_option before the first equilibration: kept and applied when the handle is created."""
    from dolfinx_eqlb_amd import _cpp as c
    from dolfinx_eqlb_amd.eqlb import _adapter as ad
    mesh, ft, G, f = _disk(70, 2, k)
    tol = bound("disk", 70, 2, k)
    Vg, Vf = ad.dg_space(mesh, k - 1, 2), ad.dg_space(mesh, k - 1, 1)
    V = ad.flux_space(mesh, k, True)
    with pytest.raises(RuntimeError, match="limit 63"):  # the default stays the refusal
        c.reconstruct_fluxes_semiexplt([c.Function(V)], [c.Function(Vg, G[0].copy())], [c.Function(Vf, f[0].copy())],
                                       _bd(c, mesh, k, ft, V, True), False)
    bd = _bd(c, mesh, k, ft, V, True)
    with pytest.raises(RuntimeError, match="unknown option"):  # checked when it is set, and not kept
        bd.set_option("large_patchs", 1)
    bd.set_option("large_patches", 1)
    flux = [c.Function(V)]
    c.reconstruct_fluxes_semiexplt(flux, [c.Function(Vg, G[0].copy())], [c.Function(Vf, f[0].copy())], bd, False)
    ref = oracle_mod.se_reconstruct(mesh, k, ft, G, f)[0]
    _check(f"module SE k={k}", flux[0].array, ref, tol)
    Vc = ad.flux_space(mesh, k, False)
    cd, nd = conforming_dofmap(mesh, k)
    bde = _bd(c, mesh, k, ft, Vc, False)
    with pytest.raises(RuntimeError, match="unknown option"):
        bde.set_option("large_patchs", 1)
    bde.set_option("large_patches", 1)
    fe = [c.Function(Vc)]
    c.reconstruct_fluxes_minimisation(c.Form([]), c.Form([]),
                                      [c.Form([c.Function(Vg, G[0].copy()), c.Function(Vf, f[0].copy())])], fe, bde)
    refe = oracle_mod.ev_reconstruct(mesh, k, ft, G, f, cd, nd)[0]
    assert np.abs(fe[0].array - refe).max() <= tol * np.abs(refe).max()


@pytest.mark.parametrize("k", [1, 2])
def test_mirrors(oracle_mod, k):
    from dolfinx_eqlb_amd.eqlb import FluxEqlbEV, FluxEqlbSE, fluxbc
    mesh, ft, G, f = _disk(70, 2, k)
    tol = bound("disk", 70, 2, k)
    bf = mesh.boundary_facets()
    prime, dual = bf[ft[0][bf] == 1], bf[ft[0][bf] == 2]
    se = FluxEqlbSE(k, mesh, [f[0]], [G[0]], large_patches=True)
    se.set_boundary_conditions([prime], [[fluxbc(0, dual, se.V_flux)]])
    se.equilibrate_fluxes()
    ref = oracle_mod.se_reconstruct(mesh, k, ft, G, f)[0]
    _check(f"FluxEqlbSE k={k}", se.get_reconstructed_fluxes(0)[0], ref, tol)
    ev = FluxEqlbEV(k, mesh, [f[0]], [G[0]], large_patches=True)
    ev.set_boundary_conditions([prime], [[fluxbc(0, dual, ev.V_flux)]])
    ev.equilibrate_fluxes()
    cd, nd = conforming_dofmap(mesh, k)
    refe = oracle_mod.ev_reconstruct(mesh, k, ft, G, f, cd, nd)[0]
    assert np.abs(ev.get_reconstructed_fluxes(0) - refe).max() <= tol * np.abs(refe).max()
    with pytest.raises(RuntimeError, match="limit 63"):
        plain = FluxEqlbSE(k, mesh, [f[0]], [G[0]])
        plain.set_boundary_conditions([prime], [[fluxbc(0, dual, plain.V_flux)]])
        plain.equilibrate_fluxes()


# ------------------------------------------------------------------------------------------------------ refusals
def test_refusals(cpp):
    mesh = create_disk(70, 1)
    ft = facet_types(mesh, None)
    st = cpp.SemiExplicitEquilibrator(cpp.DeviceMesh(mesh), 2, 2, reconstruct_stress=True)
    st.set_option("large_patches", 1)
    with pytest.raises(RuntimeError, match="stress"):
        st.set_boundary(np.repeat(ft, 2, axis=0))
    ev4 = cpp.ConstrainedMinEquilibrator(cpp.DeviceMesh(mesh), 4, 1)
    ev4.set_option("large_patches", 1)
    with pytest.raises(RuntimeError, match="RT_4"):
        ev4.set_boundary(ft)
    at = cpp.SemiExplicitEquilibrator(cpp.DeviceMesh(mesh), 2, 1)
    at.set_option("large_patches", 1)
    at.set_option("scatter", cpp.SCATTER_ATOMIC)
    at.set_boundary(ft)
    G, f = make_compatible_data(mesh, 2, ft)
    with pytest.raises(RuntimeError, match="large_patches"):
        at.equilibrate_host(G[None], f[None])
    with pytest.raises(RuntimeError, match="0 or 1"):
        at.set_option("large_patches", 2)
    # Korn constants (one wavefront per patch) are not silently computed without the hub
    at.set_option("scatter", cpp.SCATTER_SLOTS)
    with pytest.raises(RuntimeError, match="Korn"):
        at.equilibrate_host_with_kornconst(G[None], f[None])
