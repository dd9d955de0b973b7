"""Refinement of marked cells on the device (eqlb_mesh_refine_plan, eqlb_refine_*) against the numpy statement
dolfinx_eqlb_amd.mesh.refine: coordinates, cells, parent tables, counts and the tables of the refined handle bit for
bit, on the inputs of tests/refine_cases.py; four successive levels; device memory and a caller's stream; the refusals;
an equilibration on the refined handle; the pybind carrier."""

import ctypes as C

import numpy as np
import pytest

from refine_cases import NAMES, case, level_marks, sq40
from test_gpu_mesh_build import assert_is

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = -1
_REF = {}


def statement(mesh, marked):
    """(x2, cell_nodes2, parent_cell, node_parent_facet, mesh2, parent_facet, counts) of the numpy statement."""
    from dolfinx_eqlb_amd.mesh import create_mesh, parent_facets, refine_longest_edge
    x2, c2, pc, npf = refine_longest_edge(mesh, marked)
    mesh2 = create_mesh(x2, c2)
    counts = {"nnodes2": x2.shape[0], "ncells2": c2.shape[0], "nbisected": npf.size,
              "ncells_cut": int((np.bincount(pc, minlength=mesh.ncells) > 1).sum())}
    return x2, c2, pc, npf, mesh2, parent_facets(mesh, npf, mesh2), counts


def reference(name):
    if name not in _REF:
        _REF[name] = statement(*case(name))
    return _REF[name]


def assert_refinement_is(r, ref, to_host=lambda a: a):
    x2, c2, pc, npf, mesh2, pf, counts = ref
    assert r.counts == counts
    assert np.array_equal(r.dmesh.mesh.x, x2) and np.array_equal(r.dmesh.mesh.cell_nodes, c2)
    for got, want in ((r.parent_cell, pc), (r.node_parent_facet, npf), (r.parent_facet, pf)):
        got = to_host(got)
        assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want)
    assert_is(r.dmesh, mesh2)


@pytest.mark.parametrize("created", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_refinement_equals_the_statement(name, created):
    """Handles of eqlb_mesh_create_from_cells and of eqlb_mesh_create."""
    from dolfinx_eqlb_amd import cpp
    mesh, marked = case(name)
    dm = cpp.DeviceMesh(mesh) if created else cpp.DeviceMesh.from_cells(mesh.x, mesh.cell_nodes)
    assert_refinement_is(dm.refine(marked), reference(name))
    assert_is(dm, mesh)   # the handle is untouched


def test_a_hand_numbered_handle_refines_in_its_own_facet_ids():
    from dolfinx_eqlb_amd import cpp
    from test_gpu_mesh_build import shuffled_facets
    mesh, _ = shuffled_facets(case("sq3_cell5")[0], 4)
    marked = np.array([5, 20], dtype=np.int32)
    assert_refinement_is(cpp.DeviceMesh(mesh).refine(marked), statement(mesh, marked))


def test_four_levels_each_on_the_handle_of_the_level_before():
    """1/40 of the cells per level; every level refines the handle eqlb_refine_create_mesh returned."""
    from dolfinx_eqlb_amd import cpp
    mesh = sq40()
    dm, m = cpp.DeviceMesh.from_cells(mesh.x, mesh.cell_nodes), mesh
    for level in range(4):
        marked = level_marks(m.ncells, level)
        ref = statement(m, marked)
        if level == 0:   # also from a handle of eqlb_mesh_create
            assert_refinement_is(cpp.DeviceMesh(mesh).refine(marked), ref)
        r = dm.refine(marked)
        assert_refinement_is(r, ref)
        dm, m = r.dmesh, ref[4]
    assert m.ncells > 1.2 * mesh.ncells


def _device_marks(cpp, torch, ncells, stream):
    """The marked list and its count in device memory, straight from mark_doerfler_raw."""
    eta = np.random.default_rng(5).lognormal(0, 2, ncells)
    d_eta = torch.from_numpy(eta).to("cuda")
    marked = torch.full((ncells,), -7, dtype=torch.int32, device="cuda")
    nmarked = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    cpp.mark_doerfler_raw(ncells, d_eta.data_ptr(), 0.3, marked.data_ptr(), nmarked.data_ptr(), None, cpp.MEM_DEVICE,
                          stream)
    return d_eta, marked, nmarked


def test_device_memory_on_a_stream_equals_the_host_call_twice():
    import torch
    from dolfinx_eqlb_amd import cpp
    mesh = sq40()
    dm = cpp.DeviceMesh.from_cells(mesh.x, mesh.cell_nodes)
    stream = torch.cuda.Stream()   # non-blocking: not ordered against the default stream
    with torch.cuda.stream(stream):
        d_eta, marked, nmarked = _device_marks(cpp, torch, mesh.ncells, stream.cuda_stream)
        a = dm.refine((marked, nmarked), device=True, stream=stream.cuda_stream)
        b = dm.refine((marked, nmarked), device=True, stream=stream.cuda_stream)
    stream.synchronize()
    n = int(nmarked.item())
    ids = marked.cpu().numpy()[:n]
    assert 0 < n < mesh.ncells and np.all(marked.cpu().numpy()[n:] == -7)
    host = dm.refine(ids)
    ref = statement(mesh, ids)
    assert_refinement_is(host, ref)
    for r in (a, b):
        assert r.parent_cell.is_cuda and r.node_parent_facet.is_cuda and r.parent_facet.is_cuda
        assert_refinement_is(r, ref, to_host=lambda t: t.cpu().numpy())


def _plan(cpp, dm, marked, nmarked, capacity, memspace=0, null=()):
    """Raw call: (status, message, handle value)."""
    L = cpp.lib()
    sentinel = 0x5EED5EED
    h = C.c_void_p(sentinel)
    args = {"mesh": dm._h, "marked": C.c_void_p(marked), "nmarked": C.c_void_p(nmarked), "plan": C.byref(h)}
    for k in null:
        args[k] = None
    st = L.eqlb_mesh_refine_plan(args["mesh"], args["marked"], args["nmarked"], C.c_int64(capacity),
                                 C.c_int32(memspace), None, args["plan"])
    msg = L.eqlb_last_error().decode()
    if st == 0:
        L.eqlb_refine_destroy(h)
        return st, msg, None
    return int(st), msg, h.value == sentinel


def test_refusals_each_followed_by_a_valid_call():
    import torch
    from dolfinx_eqlb_amd import cpp
    mesh, good = case("sq3_cell5")
    ref = reference("sq3_cell5")
    dm = cpp.DeviceMesh.from_cells(mesh.x, mesh.cell_nodes)
    nc = mesh.ncells

    def valid():
        assert_refinement_is(dm.refine(good), ref)
        assert_is(dm, mesh)

    # nmarked = -1 as mark_doerfler_raw writes it for an array with a NaN, in device memory
    eta = np.ones(nc)
    eta[7] = np.nan
    d_eta = torch.from_numpy(eta).to("cuda")
    marked = torch.zeros(nc, dtype=torch.int32, device="cuda")
    nmarked = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    cpp.mark_doerfler_raw(nc, d_eta.data_ptr(), 0.5, marked.data_ptr(), nmarked.data_ptr(), None, cpp.MEM_DEVICE, 0)
    torch.cuda.synchronize()
    assert int(nmarked.item()) == -1
    st, msg, kept = _plan(cpp, dm, marked.data_ptr(), nmarked.data_ptr(), nc, cpp.MEM_DEVICE)
    assert st == INVALID_ARGUMENT and kept and "nmarked = -1" in msg and "eqlb_mark_doerfler" in msg, msg
    with pytest.raises(RuntimeError, match="nmarked = -1"):
        dm.refine((marked, nmarked), device=True)
    valid()
    minus = np.array([-1], dtype=np.int64)
    st, msg, kept = _plan(cpp, dm, good.ctypes.data, minus.ctypes.data, 1)
    assert st == INVALID_ARGUMENT and kept and "nmarked = -1" in msg, msg
    valid()

    # ids outside [0, ncells) among valid ones: the lowest is named, in either memory space
    for bad, named in (([3, nc, 8, nc + 5], f"cell {nc} "), ([3, nc, -1, 8, -4], "cell -4 ")):
        ids = np.array(bad, dtype=np.int32)
        n = np.array([ids.size], dtype=np.int64)
        st, msg, kept = _plan(cpp, dm, ids.ctypes.data, n.ctypes.data, ids.size)
        assert st == INVALID_ARGUMENT and kept and "eqlb_mesh_refine_plan" in msg and named in msg, msg
        d_ids, d_n = torch.from_numpy(ids).to("cuda"), torch.from_numpy(n).to("cuda")
        torch.cuda.synchronize()
        st, msg, kept = _plan(cpp, dm, d_ids.data_ptr(), d_n.data_ptr(), ids.size, cpp.MEM_DEVICE)
        assert st == INVALID_ARGUMENT and kept and named in msg, msg
        with pytest.raises(RuntimeError, match="eqlb_mesh_refine_plan"):
            dm.refine(ids)
        valid()

    # nmarked > capacity, capacity < 0
    ids = np.array([1, 2, 3], dtype=np.int32)
    n = np.array([3], dtype=np.int64)
    d_ids, d_n = torch.from_numpy(ids).to("cuda"), torch.from_numpy(n).to("cuda")
    torch.cuda.synchronize()
    for args in ((ids.ctypes.data, n.ctypes.data, 2, cpp.MEM_HOST), (d_ids.data_ptr(), d_n.data_ptr(), 2, cpp.MEM_DEVICE)):
        st, msg, kept = _plan(cpp, dm, *args)
        assert st == INVALID_ARGUMENT and kept and "capacity" in msg, msg
    st, msg, kept = _plan(cpp, dm, ids.ctypes.data, n.ctypes.data, -1)
    assert st == INVALID_ARGUMENT and kept
    st, msg, kept = _plan(cpp, dm, ids.ctypes.data, n.ctypes.data, 3, memspace=2)
    assert st == INVALID_ARGUMENT and kept and "memory space" in msg
    valid()

    # null pointers
    for null in (("mesh",), ("marked",), ("nmarked",), ("plan",)):
        st, msg, kept = _plan(cpp, dm, ids.ctypes.data, n.ctypes.data, 3, null=null)
        assert st == INVALID_ARGUMENT and "eqlb_mesh_refine_plan" in msg, (null, msg)
        assert kept or null == ("plan",)
    valid()

    # parent facets want a handle of the refined mesh
    plan = dm.refine_raw(good.ctypes.data, np.array([1], dtype=np.int64).ctypes.data, 1, cpp.MEM_HOST)
    out = np.full(mesh.nfacets, -7, dtype=np.int32)
    with pytest.raises(RuntimeError, match="eqlb_refine_parent_facets"):
        plan.parent_facets_raw(dm, out.ctypes.data, cpp.MEM_HOST)
    assert np.all(out == -7)
    # any output of the write may be left out
    nn2, nc2, nbis, ncut = plan.counts()
    only = np.zeros(nc2, dtype=np.int32)
    plan.write_raw(None, None, only.ctypes.data, None, cpp.MEM_HOST)
    assert np.array_equal(only, ref[2])
    plan.close()


@pytest.mark.parametrize("name", ["sq3_cell5", "disk"])
def test_equilibration_on_the_refined_handle(name):
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.eqlb import check_eqlb_conditions as chk
    from synthetic import facet_types, make_compatible_data
    mesh, marked = case(name)
    mesh2 = reference(name)[4]
    r = cpp.DeviceMesh.from_cells(mesh.x, mesh.cell_nodes).refine(marked)
    k = 2
    ft = facet_types(mesh2)
    G, f = make_compatible_data(mesh2, k, ft, seed=41)
    out = []
    for dm in (r.dmesh, cpp.DeviceMesh(mesh2)):
        eq = cpp.SemiExplicitEquilibrator(dm, k, 1)
        if name == "disk":
            eq.set_option("large_patches", 1)   # the hub has 70 cells and more after the refinement
        eq.set_boundary(ft)
        out.append(eq.equilibrate_host(G[None], f[None]))
    assert np.array_equal(out[0], out[1])
    assert np.all(np.isfinite(out[0])) and np.abs(out[0]).max() > 0
    res, nrm = chk.divergence_residual(mesh2, k, out[0][0], G, f)
    assert res <= 1e-10 * nrm
    # the boundary types of the old mesh carried over by parent_facet are those of the new mesh
    ft_old = facet_types(mesh)
    carried = np.where(r.parent_facet >= 0, ft_old[0][np.maximum(r.parent_facet, 0)], 0)
    assert np.array_equal(carried, ft[0])


def test_pybind_mesh_refine():
    from dolfinx_eqlb_amd import _cpp as c
    mesh, marked = case("sq3_cell5")
    x2, c2, pc, npf, mesh2, pf, counts = reference("sq3_cell5")
    base = c.Mesh.from_cells(mesh.x[:, :2], mesh.cell_nodes)
    new, parent_cell, node_parent_facet, parent_facet = base.refine(marked)
    assert (new.nnodes, new.ncells, new.nfacets) == (mesh2.nnodes, mesh2.ncells, mesh2.nfacets)
    assert np.array_equal(new.x, x2) and np.array_equal(new.cell_nodes, c2)
    assert np.array_equal(parent_cell, pc) and np.array_equal(node_parent_facet, npf)
    assert np.array_equal(parent_facet, pf)
    assert np.array_equal(new.boundary_facets(), mesh2.boundary_facets())
    assert np.array_equal(new.find_facets(mesh2.facet_nodes), np.arange(mesh2.nfacets))
    with pytest.raises(RuntimeError, match="marked cell"):
        base.refine(np.array([mesh.ncells], dtype=np.int32))
