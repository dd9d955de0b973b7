"""Weak symmetry and Korn constants on vertex patches of more than 63 cells (options "large_patches" +
"large_patches_stress": k_se_weaksym_large, one workgroup per patch; k_korn_patch on the large-patch SoA) against the
oracle: polar disks whose hub has 64 ... 257 cells, half annuli whose hub lies on the boundary, both scatter routes,
lower data degrees, two hubs, node masks, device memory on a caller's stream, the FluxEqlbSE mirror, the refusals.

Bound of every device-vs-oracle comparison, relative to max |oracle|: max(1e-10, 10 x the discrepancy recorded for the
case in tests/test_large_patches_stress_oracle.py) - 1e-10 is run_stress's figure for the one-wave path
(tests/test_gpu_stress_large_patches.py), the record is what two elimination orders of the hub's weak-symmetry problem
differ by on the CPU already, the factor 10 allows for the device's third order.  Asymmetry moments below
1e-11 max(1, scale), run_stress's figure as well.  Every handle sets both options."""

import functools

import numpy as np
import pytest

import galerkin as gk
from dolfinx_eqlb_amd.eqlb import check_eqlb_conditions as chk
from dolfinx_eqlb_amd.mesh import create_disk, create_mesh, create_unit_square
from synthetic import facet_types, make_compatible_stress_data
from test_gpu_stress_large_patches import big_double_fan_mesh, flux_types
from test_large_patches_oracle import half_annulus, hub_node
from test_large_patches_stress_oracle import (ANNULUS_LAYOUTS, annulus_types, hub_stress_discrepancy, stress_case)
from test_oracle_stress import asym_moments

pytestmark = pytest.mark.gpu


def bound(kind, n, layout, k):
    return max(1e-10, 10.0 * hub_stress_discrepancy(kind, n, layout, k))


@pytest.fixture(scope="module")
def cpp():
    from dolfinx_eqlb_amd import cpp as c
    assert c.device_count() >= 1, "GPU tests need a HIP device"
    return c


_REF = {}


def _ref(oracle_mod, key, mesh, k, ft, G, f, **kw):
    """Oracle results are computed once per case and shared (never modified)."""
    if key not in _REF:
        _REF[key] = oracle_mod.se_reconstruct(mesh, k, ft, G, f, stress=True, **kw)
        _REF[key].setflags(write=False)
    return _REF[key]


def _handle(cpp, mesh, k, nrhs=2, d=None, stress=True, scatter=None, accumulate=1):
    eq = cpp.SemiExplicitEquilibrator(cpp.DeviceMesh(mesh), k, nrhs, degree_dg=d, reconstruct_stress=stress)
    if scatter is not None:
        eq.set_option("scatter", scatter)
    eq.set_option("accumulate", accumulate)
    eq.set_option("large_patches", 1)
    eq.set_option("large_patches_stress", 1)
    return eq


def _check(name, mesh, k, x, ref, G, f, tol, d=None, symmetric=True):
    scale = np.abs(ref).max()
    err = np.abs(x - ref).max() / scale
    asym = np.abs(asym_moments(mesh, k, x)[1]).max()
    print(f"{name}: device vs oracle {err:.2e} (bound {tol:.1e}), asymmetry {asym:.2e}")
    assert np.isfinite(x).all() and err <= tol, (name, err, tol)
    if symmetric:
        assert asym < 1e-11 * max(1.0, scale)
    else:
        # data that miss the moment balance of the weak-symmetry step: the oracle leaves an asymmetry, the device the same
        left = asym_moments(mesh, k, ref)[1]
        assert np.abs(left).max() > 1e-6 and np.abs(asym_moments(mesh, k, x)[1] - left).max() < 1e-11 * max(1.0, scale)
    for r in range(2):
        res, nrm = chk.divergence_residual(mesh, k, x[r], G[r], f[r], degree_dg=d)
        assert res <= 1e-10 * nrm
        assert chk.check_jump_condition(mesh, k, x[r], G[r], degree_dg=d, atol=1e-9)


def _run(cpp, oracle_mod, name, key, mesh, k, ft, G, f, tol, nlarge, bv=None, scatter=None):
    ref = _ref(oracle_mod, key, mesh, k, ft, G, f, boundary_values=bv)
    eq = _handle(cpp, mesh, k, scatter=scatter)
    eq.set_boundary(ft, boundary_values=bv)
    assert eq.large_patch_info() == nlarge
    x = eq.equilibrate_host(G, f)
    _check(name, mesh, k, x, ref, G, f, tol)
    if bv is not None:
        for r in range(2):
            assert chk.boundary_flux_residual(mesh, k, x[r], G[r], np.nonzero(ft[r] == 2)[0],
                                             boundary_values=bv[r]) \
                <= 1e-10 * max(1.0, np.abs(ref).max())
    assert np.array_equal(x, eq.equilibrate_host(G, f))  # a second call gives the same bits
    return x


# ------------------------------------------------------------------------------------------- device against oracle
DISKS = [(n, lay, k) for lay in ("dirichlet", "traction") for n in (64, 65, 129) for k in (2, 3, 4) if k < 4 or n == 64] \
    + [(257, "dirichlet", 2)]


@pytest.mark.parametrize("n,layout,k", DISKS, ids=[f"ns{n}-{lay}-k{k}" for n, lay, k in DISKS])
def test_disk(cpp, oracle_mod, n, layout, k):
    mesh, ft, G, f = stress_case("disk", n, layout, k)
    _run(cpp, oracle_mod, f"disk {n} {layout} k={k}", ("disk", n, layout, k), mesh, k, ft, G, f,
         bound("disk", n, layout, k), (1, n))


@pytest.mark.parametrize("k", [2, 3, 4])
@pytest.mark.parametrize("layout", ANNULUS_LAYOUTS)
def test_boundary_fan(cpp, oracle_mod, k, layout):
    mesh, ft, G, f = stress_case("annulus", 64, layout, k)
    _run(cpp, oracle_mod, f"annulus 64 {layout} k={k}", ("annulus", 64, layout, k), mesh, k, ft, G, f,
         bound("annulus", 64, layout, k), (1, 64))


@pytest.mark.parametrize("k", [2, 3, 4])
@pytest.mark.parametrize("kind", ["disk", "annulus"])
def test_galerkin_inhomogeneous_tractions(cpp, oracle_mod, kind, k):
    """A P_k elasticity solution with prescribed (non-zero) tractions: boundary values on the stress rows."""
    if kind == "disk":
        mesh = create_disk(64, 2, shuffle_seed=7)
        ft = flux_types(mesh, [lambda m: m[:, 1] > 0.0] * 2)
        layout = "traction"
    else:
        mesh = half_annulus(64)
        ft = annulus_types(mesh, "both_meanvalue")
        layout = "both_meanvalue"
    G, f, bv = gk.solve_elasticity(mesh, k, ft, seed=31 * k + 64)
    assert np.abs(bv).max() > 1e-3
    _run(cpp, oracle_mod, f"galerkin {kind} 64 k={k}", ("galerkin", kind, k), mesh, k, ft, G, f,
         bound(kind, 64, layout, k), (1, 64), bv=bv)


# --------------------------------------------------------------------------------------------------- scatter routes
@pytest.mark.parametrize("n", [64, 65, 129, 257])
def test_scatter_routes(cpp, oracle_mod, n):
    """RT_2 with DG_1 data and no flux BC on the stress rows: the slot route, and SCATTER_AUTO = the fused tiled stress
    launch, for which the hub is a masked node whose rows the large-patch kernels add behind it."""
    k = 2
    mesh, ft, G, f = stress_case("disk", n, "dirichlet", k)
    ref = _ref(oracle_mod, ("disk", n, "dirichlet", k), mesh, k, ft, G, f)
    tol = bound("disk", n, "dirichlet", k)
    for scatter in (cpp.SCATTER_SLOTS, None):
        eq = _handle(cpp, mesh, k, scatter=scatter)
        eq.set_boundary(ft)
        assert eq.large_patch_info() == (1, n)
        x = eq.equilibrate_host(G, f)
        _check(f"disk {n} scatter={scatter}", mesh, k, x, ref, G, f, tol)
        assert np.array_equal(x, eq.equilibrate_host(G, f))


@pytest.mark.parametrize("scatter", [0, None])
def test_accumulate_0(cpp, oracle_mod, scatter):
    """accumulate = 0 overwrites a pre-filled vector, accumulate = 1 adds to it."""
    k, n = 2, 65
    mesh, ft, G, f = stress_case("disk", n, "dirichlet", k)
    ref = _ref(oracle_mod, ("disk", n, "dirichlet", k), mesh, k, ft, G, f)
    pre = np.full(ref.shape, 0.375)
    for acc in (0, 1):
        eq = _handle(cpp, mesh, k, scatter=scatter, accumulate=acc)
        eq.set_boundary(ft)
        x = eq.equilibrate_host(G, f, pre.copy()) - (pre if acc else 0.0)
        _check(f"accumulate={acc} scatter={scatter}", mesh, k, x, ref, G, f, bound("disk", n, "dirichlet", k))


# ---------------------------------------------------------------------------------------------------- other cases
@pytest.mark.parametrize("k,d", [(2, 0), (3, 1)])
def test_lower_data_degree(cpp, oracle_mod, k, d):
    """DG_0 data at RT_2, DG_1 data at RT_3: Galerkin elasticity in P_{d+1} (as tests/test_gpu_lower_degree.py),
    Dirichlet rim.  P1 Galerkin stresses (d = 0) do not satisfy the moment balance against x hat_a, which is not in P1:
    the oracle leaves an asymmetry there (tests/test_gpu_lower_degree.py::test_stress_matches_oracle asserts the weak
    symmetry for d >= 1 only); at d = 0 the device has to leave the same one."""
    mesh = create_disk(64, 2, shuffle_seed=7)
    ft = np.repeat(facet_types(mesh, None), 2, axis=0)
    G, f, _ = gk.solve_elasticity(mesh, d + 1, ft, seed=3, traction=lambda r, x, y: 0.0 * x)
    ref = oracle_mod.se_reconstruct(mesh, k, ft, G, f, degree_dg=d, stress=True)
    eq = _handle(cpp, mesh, k, d=d)
    eq.set_boundary(ft)
    assert eq.large_patch_info() == (1, 64)
    x = eq.equilibrate_host(G, f)
    _check(f"disk 64 k={k} d={d}", mesh, k, x, ref, G, f, bound("disk", 64, "dirichlet", k), d=d, symmetric=d >= 1)
    assert np.array_equal(x, eq.equilibrate_host(G, f))


def _two_fans():
    """Two disjoint disks in one mesh: hubs of 64 and of 65 cells."""
    a, b = create_disk(64, 2, shuffle_seed=3), create_disk(65, 2, shuffle_seed=4)
    xb = b.x[:, :2] + np.array([3.0, 0.0])
    x = np.concatenate([a.x[:, :2], xb])
    cells = np.concatenate([a.cell_nodes, b.cell_nodes + a.nnodes]).astype(np.int32)
    return create_mesh(x, cells)


@pytest.mark.parametrize("k", [2, 3])
def test_two_large_patches_in_one_call(cpp, oracle_mod, k):
    mesh = _two_fans()
    ft = np.repeat(facet_types(mesh, lambda x: x[:, 1] > 0.0), 2, axis=0)
    G, f = make_compatible_stress_data(mesh, k, ft)
    tol = max(bound("disk", 64, "traction", k), bound("disk", 65, "traction", k))
    _run(cpp, oracle_mod, f"two fans k={k}", ("two", k), mesh, k, ft, G, f, tol, (2, 65))


@pytest.mark.parametrize("k", [2, 3])
def test_hub_masked_out_is_the_one_wave_path(cpp, k):
    """Without the hub nothing is left for the large-patch kernels: the same bits as a handle without the options."""
    mesh, ft, G, f = stress_case("disk", 64, "traction", k)
    mask = np.ones(mesh.nnodes, dtype=np.uint8)
    mask[hub_node(mesh)] = 0
    eq = _handle(cpp, mesh, k)
    eq.set_boundary(ft, node_mask=mask)
    assert eq.large_patch_info() == (0, 0)
    plain = cpp.SemiExplicitEquilibrator(cpp.DeviceMesh(mesh), k, 2, reconstruct_stress=True)
    plain.set_boundary(ft, node_mask=mask)
    x = eq.equilibrate_host(G, f)
    assert np.abs(x).max() > 0.0 and np.array_equal(x, plain.equilibrate_host(G, f))


@pytest.mark.parametrize("k,layout", [(2, "dirichlet"), (3, "traction")])
def test_device_pointers_on_a_user_stream(cpp, k, layout):
    """Inputs produced late on a non-blocking stream (as tests/test_gpu_streams.py), the first call on a fresh handle
    included: check_status is OK and the result equals the host-memory call of a second handle bit for bit."""
    import torch
    mesh, ft, G, f = stress_case("disk", 65, layout, k)

    def handle():
        h = _handle(cpp, mesh, k)
        h.set_boundary(ft)
        assert h.large_patch_info() == (1, 65)
        return h

    ref = handle().equilibrate_host(G, f)
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    g_src, f_src = torch.from_numpy(G).to(dev), torch.from_numpy(f).to(dev)
    g_dev, f_dev = torch.full_like(g_src, float("nan")), torch.full_like(f_src, float("nan"))
    x_dev = torch.full(ref.shape, float("nan"), dtype=torch.float64, device=dev)
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


# -------------------------------------------------------------------------------------------------- Korn constants
@functools.lru_cache(maxsize=None)
def _korn_mesh(kind, n):
    mesh = create_disk(n, 2, shuffle_seed=7) if kind == "disk" else half_annulus(n)
    sel = (lambda x: x[:, 1] > 0.0) if kind == "disk" else (lambda p: np.abs(p[:, 1]) < 1e-12)
    return mesh, np.repeat(facet_types(mesh, sel), 2, axis=0)


@pytest.mark.parametrize("stress", [False, True])
@pytest.mark.parametrize("kind,n", [("disk", 64), ("disk", 100), ("annulus", 64)])
def test_korn_constants(cpp, oracle_mod, kind, n, stress):
    k = 2
    mesh, ft = _korn_mesh(kind, n)
    G, f = make_compatible_stress_data(mesh, k, ft)
    ref = oracle_mod.se_korn(mesh, ft)
    eq = _handle(cpp, mesh, k, stress=stress)
    eq.set_boundary(ft)
    assert eq.large_patch_info() == (1, n)
    x, korn = eq.equilibrate_host_with_kornconst(G, f)
    assert np.allclose(korn, ref, rtol=1e-12, atol=0.0)
    assert np.allclose(eq.kornconst_host(), ref, rtol=1e-12, atol=0.0)
    xs = oracle_mod.se_reconstruct(mesh, k, ft, G, f, stress=stress)
    assert np.abs(x - xs).max() <= 1e-10 * np.abs(xs).max()


# ---------------------------------------------------------------------------------------------------------- mirror
def test_mirror_stress_korn(oracle_mod):
    """FluxEqlbSE with stress, Korn constants and large_patches=True sets both options."""
    from dolfinx_eqlb_amd.eqlb.FluxEqlbSE import FluxEqlbSE, fluxbc
    k = 2
    mesh = create_disk(70, 2, shuffle_seed=7)
    bf = mesh.boundary_facets()
    mid = mesh.x[mesh.facet_nodes[bf]].mean(axis=1)[:, :2]
    trac, disp = bf[mid[:, 1] > 0.0], bf[~(mid[:, 1] > 0.0)]
    ft = np.zeros((2, mesh.nfacets), dtype=np.int8)
    ft[:, disp] = 1
    ft[:, trac] = 2
    G, f, bv = gk.solve_elasticity(mesh, k, ft, seed=77, traction=lambda r, x, y: 0.0 * x)
    eq = FluxEqlbSE(k, mesh, [f[0], f[1]], [G[0], G[1]], True, True, large_patches=True)
    eq.set_boundary_conditions([disp, disp], [[fluxbc(0, trac, eq.V_flux)], [fluxbc(0, trac, eq.V_flux)]])
    assert np.array_equal(eq.facet_type, ft)
    eq.equilibrate_fluxes()
    x = eq.list_flux
    ref = oracle_mod.se_reconstruct(mesh, k, ft, G, f, stress=True)
    scale = np.abs(ref).max()
    assert np.abs(x - ref).max() <= bound("disk", 70, "traction", k) * scale
    for r in range(2):
        res, nrm = chk.divergence_residual(mesh, k, x[r], G[r], f[r])
        assert res <= 1e-10 * max(nrm, scale)
        assert chk.jump_residual(mesh, k, x[r], G[r]) <= 1e-9 * scale
        assert chk.boundary_flux_residual(mesh, k, x[r], G[r], trac) <= 1e-10 * max(1.0, scale)
    assert np.abs(asym_moments(mesh, k, x)[1]).max() < 1e-11 * max(1.0, scale)
    assert chk.check_weak_symmetry_condition(mesh, k, x)
    assert np.allclose(eq.get_korn_constants(), np.sqrt(oracle_mod.se_korn(mesh, ft)), rtol=1e-12)
    with pytest.raises(RuntimeError, match="limit 63"):  # the default stays the refusal
        plain = FluxEqlbSE(k, mesh, [f[0], f[1]], [G[0], G[1]], True, True)
        plain.set_boundary_conditions([disp, disp], [[fluxbc(0, trac, plain.V_flux)], [fluxbc(0, trac, plain.V_flux)]])
        plain.equilibrate_fluxes()


# ----------------------------------------------------------------------------------------------- nothing else moves
@pytest.mark.parametrize("k", [2, 3])
def test_regular_mesh_is_untouched(cpp, k):
    """Without a large patch the option changes neither the launches (eqlb_se_tiling_blocks) nor one bit."""
    mesh = create_unit_square(12, shuffle_seed=2, perturb=0.15)
    ft = np.repeat(facet_types(mesh, None), 2, axis=0)
    G, f = make_compatible_stress_data(mesh, k, ft)
    out = []
    for opt in (0, 1):
        eq = cpp.SemiExplicitEquilibrator(cpp.DeviceMesh(mesh), k, 2, reconstruct_stress=True)
        eq.set_option("large_patches", 1)
        eq.set_option("large_patches_stress", opt)
        eq.set_boundary(ft)
        assert eq.large_patch_info() == (0, 0)
        x, korn = eq.equilibrate_host_with_kornconst(G, f)
        out.append((eq.tiling_blocks(), x, korn))
    assert out[0][0] == out[1][0]
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])


# -------------------------------------------------------------------------------------------------------- refusals
def test_option_values_and_default_refusals(cpp):
    mesh = create_disk(70, 1)
    ft = np.repeat(facet_types(mesh, None), 2, axis=0)
    st = cpp.SemiExplicitEquilibrator(cpp.DeviceMesh(mesh), 2, 2, reconstruct_stress=True)
    with pytest.raises(RuntimeError, match="0 or 1"):
        st.set_option("large_patches_stress", 2)
    # the option alone does nothing: "large_patches" decides whether a large patch is accepted at all
    st.set_option("large_patches_stress", 1)
    with pytest.raises(RuntimeError, match="limit 63"):
        st.set_boundary(ft)
    ev = cpp.ConstrainedMinEquilibrator(cpp.DeviceMesh(mesh), 2, 1)
    with pytest.raises(RuntimeError, match="unknown option"):  # EV handles do not have the key
        ev.set_option("large_patches_stress", 1)


@pytest.mark.parametrize("order", [0, 1])
def test_large_patch_in_a_group_is_refused(cpp, order):
    """Tractions on the whole boundary at RT_2: the hub of 64 cells is the internal patch of a group of boundary
    patches (se/reconstruction.hpp:170-234) - refused, never silently wrong."""
    mesh = big_double_fan_mesh(61, order)
    assert np.diff(mesh.node_cells_offsets).max() == 64
    ft = np.repeat(facet_types(mesh, lambda p: np.ones(len(p), dtype=bool)), 2, axis=0)
    eq = _handle(cpp, mesh, 2)
    with pytest.raises(RuntimeError, match="group"):
        eq.set_boundary(ft)
    # the code of the C ABI: EQLB_ERR_UNSUPPORTED
    import ctypes as C
    ftc = np.ascontiguousarray(ft, dtype=np.int8)
    st = cpp.lib().eqlb_se_set_boundary(eq._h, ftc.ctypes.data_as(C.c_void_p), None, None)
    assert st == -3 and b"group" in cpp.lib().eqlb_last_error()
