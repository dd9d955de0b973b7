"""Mesh connectivity built on the device (eqlb_mesh_create_from_cells) against dolfinx_eqlb_amd.mesh.create_mesh, the
statement of the numbering: every table bit for bit, in host and device memory, the entries that read a handle back
(export, boundary facets, facet ids of node pairs), the refusals, and the identity of everything downstream."""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TABLES = ("cell_facets", "facet_nodes", "facet_cells_offsets", "facet_cells", "node_cells_offsets", "node_cells",
          "node_facets_offsets", "node_facets", "facet_perm")
TOPOLOGY = ["hole", "two_holes", "lshape", "two_parts", "bowtie"]
NAMES = ["sq3", "left", "right", "disk70"] + TOPOLOGY + ["delaunay", "unused_nodes", "sq40", "sq182_permuted"]
INVALID_ARGUMENT = -1


def _left_diagonal(n):
    """n x n squares cut along the diagonal from (i+1, j) to (i, j+1)."""
    from dolfinx_eqlb_amd.mesh import create_mesh
    ii, jj = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="xy")
    x = np.stack([ii.ravel() / n, jj.ravel() / n], axis=1)
    ci, cj = [a.ravel() for a in np.meshgrid(np.arange(n), np.arange(n), indexing="xy")]
    v00 = cj * (n + 1) + ci
    v10, v01, v11 = v00 + 1, v00 + n + 1, v00 + n + 2
    cells = np.stack([np.stack([v00, v10, v01], 1), np.stack([v10, v11, v01], 1)], axis=1).reshape(-1, 3)
    return create_mesh(x, cells.astype(np.int32))


def _permuted(mesh, seed):
    """The same mesh with the node numbers randomly permuted."""
    from dolfinx_eqlb_amd.mesh import create_mesh
    perm = np.random.default_rng(seed).permutation(mesh.nnodes).astype(np.int32)  # new number of old node i
    x = np.empty((mesh.nnodes, 2))
    x[perm] = mesh.x[:, :2]
    return create_mesh(x, perm[mesh.cell_nodes])


def _max_key(mesh):
    fn = mesh.facet_nodes.astype(np.int64)
    return int((fn.min(axis=1) * mesh.nnodes + fn.max(axis=1)).max())


_REF = {}


def reference(name):
    """create_mesh of the named input - the oracle; built once."""
    if name in _REF:
        return _REF[name]
    from dolfinx_eqlb_amd.mesh import create_disk, create_mesh, create_unit_square
    if name == "sq3":
        m = create_unit_square(3, shuffle_seed=1)
        assert m.ncells == 36
    elif name == "left":
        m = _left_diagonal(3)
    elif name == "right":
        m = create_unit_square(3, diagonal="right")
    elif name == "disk70":
        m = create_disk(70, 1)
        assert np.diff(m.node_cells_offsets).max() == 70
    elif name in TOPOLOGY:
        from topology_meshes import mesh_of
        m = mesh_of(name)
    elif name == "delaunay":
        from test_fuzz import random_case
        m = random_case(3, 1, 1)[0]
    elif name == "unused_nodes":   # nodes 3, 5 and 6 belong to no cell: empty rows in the middle and at the end
        x = np.array([[0, 0], [1, 0], [0, 1], [5, 5], [1, 1], [6, 6], [7, 7]], dtype=np.float64)
        m = create_mesh(x, np.array([[0, 1, 2], [2, 1, 4]], dtype=np.int32))
        assert np.array_equal(np.diff(m.node_cells_offsets), [1, 2, 2, 0, 1, 0, 0])
    elif name == "sq40":            # 19 200 keys: several blocks of the sort and of the scans
        m = create_unit_square(40, shuffle_seed=2)
        assert 3 * m.ncells == 19200
    elif name == "sq182_permuted":  # facet keys beyond 32 bits
        base = create_unit_square(182, shuffle_seed=3)
        assert _max_key(base) < 2 ** 32   # (the centre nodes are numbered last)
        m = _permuted(base, 3)
        assert _max_key(m) >= 2 ** 32
    else:
        raise KeyError(name)
    _REF[name] = m
    return m


def assert_is(dm, ref):
    assert dm.counts() == (ref.nnodes, ref.ncells, ref.nfacets)
    assert dm.max_patch_cells == int(np.diff(ref.node_cells_offsets).max())
    t = dm.export()
    for key in TABLES:
        want = getattr(ref, key)
        assert t[key].dtype == want.dtype and t[key].shape == want.shape, key
        assert np.array_equal(t[key], want), key
        assert np.array_equal(getattr(dm.mesh, key), want), key
    assert np.array_equal(dm.mesh.x, ref.x) and np.array_equal(dm.mesh.cell_nodes, ref.cell_nodes)


_HANDLES = {}


def handle(name):
    """DeviceMesh.from_cells of the named input from host arrays; built once."""
    if name not in _HANDLES:
        from dolfinx_eqlb_amd import cpp
        ref = reference(name)
        _HANDLES[name] = cpp.DeviceMesh.from_cells(ref.x[:, :2], ref.cell_nodes)
    return _HANDLES[name]


def shuffled_facets(mesh, seed):
    """The mesh with its facets renumbered at random (and the rows of node_facets no longer ascending): what a caller
    with a numbering of their own hands to eqlb_mesh_create."""
    from dolfinx_eqlb_amd.mesh import Mesh
    p = np.random.default_rng(seed).permutation(mesh.nfacets).astype(np.int32)  # new id of old facet f
    inv = np.argsort(p)
    cnt = np.diff(mesh.facet_cells_offsets)[inv]
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    fc = np.concatenate([mesh.facet_cells[mesh.facet_cells_offsets[f]:mesh.facet_cells_offsets[f + 1]] for f in inv])
    return Mesh(mesh.x, mesh.cell_nodes, p[mesh.cell_facets], mesh.facet_nodes[inv], off, fc.astype(np.int32),
                mesh.node_cells_offsets, mesh.node_cells, mesh.node_facets_offsets, p[mesh.node_facets],
                mesh.facet_perm), p


# ---- 1, 2: the tables ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_tables_equal_create_mesh(name):
    assert_is(handle(name), reference(name))


@pytest.mark.parametrize("name", NAMES)
def test_tables_from_device_memory_on_a_stream(name):
    import torch
    from dolfinx_eqlb_amd import cpp
    ref = reference(name)
    stream = torch.cuda.Stream()   # non-blocking: not ordered against the default stream
    with torch.cuda.stream(stream):
        dx = torch.from_numpy(ref.x).to("cuda")
        dc = torch.from_numpy(ref.cell_nodes).to("cuda")
        dm = cpp.DeviceMesh.from_cells(dx, dc, device=True, stream=stream.cuda_stream)
        again = cpp.DeviceMesh.from_cells(dx, dc, device=True, stream=stream.cuda_stream)
    assert_is(dm, ref)
    assert np.array_equal(dx.cpu().numpy(), ref.x) and np.array_equal(dc.cpu().numpy(), ref.cell_nodes)
    a, b = dm.export(), again.export()
    for key in TABLES:
        assert np.array_equal(a[key], b[key]), key
    assert again.max_patch_cells == dm.max_patch_cells


# ---- 3: export of a handle of eqlb_mesh_create --------------------------------------------------------------------
def test_export_round_trip_of_a_created_handle():
    import torch
    from dolfinx_eqlb_amd import cpp
    mesh, _ = shuffled_facets(reference("sq3"), 4)
    dm = cpp.DeviceMesh(mesh)
    assert dm.counts() == (mesh.nnodes, mesh.ncells, mesh.nfacets)
    t = dm.export()
    for key in TABLES:
        assert np.array_equal(t[key], getattr(mesh, key)), key
    dev = {key: torch.full((getattr(mesh, key).size,), 9, device="cuda",
                           dtype=torch.uint8 if key == "facet_perm" else torch.int32) for key in TABLES}
    st = torch.cuda.current_stream().cuda_stream
    dm.export_raw(**{key: v.data_ptr() for key, v in dev.items()}, memspace=cpp.MEM_DEVICE, stream=st)
    torch.cuda.synchronize()
    for key in TABLES:
        assert np.array_equal(dev[key].cpu().numpy(), getattr(mesh, key).ravel()), key
    # any output may be left out
    only = np.zeros_like(mesh.facet_nodes)
    dm.export_raw(facet_nodes=only.ctypes.data, memspace=cpp.MEM_HOST)
    assert np.array_equal(only, mesh.facet_nodes)


# ---- 4: everything downstream ---------------------------------------------------------------------------------------
def _downstream(cpp, dm, ft, G, f, G3, f3, Gs, fs):
    out = {}
    for label, scatter in (("se2_tiled", cpp.SCATTER_TILED), ("se2_slots", cpp.SCATTER_SLOTS)):
        eq = cpp.SemiExplicitEquilibrator(dm, 2, 1)
        eq.set_option("scatter", scatter)
        eq.set_boundary(ft)
        out[label] = eq.equilibrate_host(G, f)
    eq = cpp.SemiExplicitEquilibrator(dm, 3, 1)
    eq.set_boundary(ft)
    out["se3"] = eq.equilibrate_host(G3, f3)
    ev = cpp.ConstrainedMinEquilibrator(dm, 2, 1)
    ev.set_boundary(ft)
    out["ev2"] = ev.equilibrate_host(G, f)
    ft2 = np.repeat(ft, 2, axis=0)
    eq = cpp.SemiExplicitEquilibrator(dm, 2, 2, reconstruct_stress=True, estimate_korn=True)
    eq.set_boundary(ft2)
    out["stress2"], out["korn"] = eq.equilibrate_host_with_kornconst(Gs, fs)
    return out


@pytest.mark.parametrize("name", ["hole", "sq6"])
def test_downstream_results_are_bitwise_those_of_a_created_handle(oracle_mod, name):
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.mesh import create_unit_square
    from synthetic import facet_types, make_compatible_data, make_compatible_stress_data
    if name == "hole":
        from topology_meshes import mesh_of
        mesh = mesh_of("hole")
    else:
        mesh = create_unit_square(6, shuffle_seed=5, perturb=0.2)
    ft = facet_types(mesh, None)
    G, f = [a[None] for a in make_compatible_data(mesh, 2, ft, seed=31)]
    G3, f3 = [a[None] for a in make_compatible_data(mesh, 3, ft, seed=32)]
    Gs, fs = make_compatible_stress_data(mesh, 2, np.repeat(ft, 2, axis=0))
    built = cpp.DeviceMesh.from_cells(mesh.x, mesh.cell_nodes)
    assert_is(built, mesh)
    a = _downstream(cpp, cpp.DeviceMesh(mesh), ft, G, f, G3, f3, Gs, fs)
    b = _downstream(cpp, built, ft, G, f, G3, f3, Gs, fs)
    for key in a:
        assert np.array_equal(a[key], b[key]), key
        assert np.all(np.isfinite(b[key])) and np.abs(b[key]).max() > 0, key
    ref = oracle_mod.se_reconstruct(mesh, 2, ft, G, f)
    for key in ("se2_tiled", "se2_slots"):   # the bound of tests/test_gpu_parity.py
        assert np.abs(b[key] - ref).max() <= 1e-11 * np.abs(ref).max(), key


# ---- 5: boundary facets -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_boundary_facets(name):
    ref = reference(name)
    got = handle(name).boundary_facets()
    assert got.dtype == np.int32 and np.array_equal(got, ref.boundary_facets())


def test_boundary_facets_of_a_hand_numbered_mesh_and_capacity():
    import torch
    from dolfinx_eqlb_amd import cpp
    base = reference("sq3")
    mesh, p = shuffled_facets(base, 9)
    dm = cpp.DeviceMesh(mesh)
    want = np.sort(p[base.boundary_facets()])
    assert np.array_equal(want, mesh.boundary_facets()) and want.size == 12
    assert np.array_equal(dm.boundary_facets(), want)
    # undersized: refused, the count reported, nothing written - in both memory spaces
    buf = np.full(want.size, -7, dtype=np.int32)
    st, n = dm.boundary_facets_raw(buf.ctypes.data, want.size - 1, memspace=cpp.MEM_HOST)
    assert (st, n) == (INVALID_ARGUMENT, want.size) and np.all(buf == -7)
    assert "eqlb_mesh_boundary_facets" in cpp.lib().eqlb_last_error().decode()
    dbuf = torch.full((want.size,), -7, dtype=torch.int32, device="cuda")
    cur = torch.cuda.current_stream().cuda_stream
    st, n = dm.boundary_facets_raw(dbuf.data_ptr(), 0, memspace=cpp.MEM_DEVICE, stream=cur)
    assert (st, n) == (INVALID_ARGUMENT, want.size) and bool((dbuf == -7).all())
    st, n = dm.boundary_facets_raw(dbuf.data_ptr(), want.size, memspace=cpp.MEM_DEVICE, stream=cur)
    assert (st, n) == (0, want.size) and np.array_equal(dbuf.cpu().numpy(), want)
    # larger than needed: the tail is not touched
    big = np.full(want.size + 3, -7, dtype=np.int32)
    st, n = dm.boundary_facets_raw(big.ctypes.data, big.size, memspace=cpp.MEM_HOST)
    assert (st, n) == (0, want.size) and np.array_equal(big[:n], want) and np.all(big[n:] == -7)


# ---- 6: facet ids of node pairs -----------------------------------------------------------------------------------
def _check_find_facets(dm, mesh):
    import torch
    from dolfinx_eqlb_amd import cpp
    ids = np.arange(mesh.nfacets, dtype=np.int32)
    assert np.array_equal(dm.find_facets(mesh.facet_nodes), ids)
    assert np.array_equal(dm.find_facets(mesh.facet_nodes[:, ::-1]), ids)
    # nodes that share no edge: node 0 and every node that is not its neighbour (and itself)
    nb = np.unique(mesh.facet_nodes[np.any(mesh.facet_nodes == 0, axis=1)])
    far = np.setdiff1d(np.arange(mesh.nnodes), nb)
    assert far.size > 0
    pairs = np.concatenate([np.stack([np.zeros_like(far), far], 1), np.stack([far, np.zeros_like(far)], 1),
                            [[0, 0], [-1, 1], [1, -1], [mesh.nnodes, 0], [0, mesh.nnodes], [2 ** 31 - 1, 1],
                             [-2 ** 31, -2 ** 31]]]).astype(np.int32)
    assert np.all(dm.find_facets(pairs) == -1)
    mixed = np.concatenate([pairs[:3], mesh.facet_nodes[:5], pairs[-3:]]).astype(np.int32)
    want = np.concatenate([[-1] * 3, ids[:5], [-1] * 3])
    assert np.array_equal(dm.find_facets(mixed), want)
    dp = torch.from_numpy(mixed).to("cuda")
    out = torch.full((mixed.shape[0],), -5, dtype=torch.int32, device="cuda")
    dm.find_facets_raw(mixed.shape[0], dp.data_ptr(), out.data_ptr(), memspace=cpp.MEM_DEVICE,
                       stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    assert dm.find_facets(np.zeros((0, 2), dtype=np.int32)).size == 0


def test_find_facets_on_a_built_handle():
    for name in ("sq3", "bowtie", "unused_nodes"):
        _check_find_facets(handle(name), reference(name))


def test_find_facets_assumes_nothing_about_the_facet_order():
    from dolfinx_eqlb_amd import cpp
    mesh, _ = shuffled_facets(reference("sq3"), 11)
    assert not np.array_equal(mesh.facet_nodes, reference("sq3").facet_nodes)
    rows = [mesh.node_facets[a:b] for a, b in zip(mesh.node_facets_offsets[:-1], mesh.node_facets_offsets[1:])]
    assert any(np.any(np.diff(r) < 0) for r in rows)   # rows that are not ascending
    _check_find_facets(cpp.DeviceMesh(mesh), mesh)


# ---- 7: refusals -----------------------------------------------------------------------------------------------------
def _malformed():
    """name -> (cells, text the message must contain) on the 36-cell mesh."""
    ref = reference("sq3")
    nn = ref.nnodes
    out = {}
    # an interior edge (a, b) of the cells c0, c1 put into a third cell as well
    f = int(np.nonzero(np.diff(ref.facet_cells_offsets) == 2)[0][0])
    a, b = ref.facet_nodes[f]
    own = ref.facet_cells[ref.facet_cells_offsets[f]:ref.facet_cells_offsets[f] + 2]
    j = [c for c in range(ref.ncells) if c not in own][-1]
    c3 = [v for v in range(nn) if v not in (a, b)][-1]
    cells = ref.cell_nodes.copy()
    cells[j] = [a, c3, b]
    lo = np.minimum(cells[:, [1, 0, 0]], cells[:, [2, 2, 1]]).astype(np.int64)
    hi = np.maximum(cells[:, [1, 0, 0]], cells[:, [2, 2, 1]]).astype(np.int64)
    keys, cnt = np.unique(lo * nn + hi, return_counts=True)
    first = int(keys[cnt > 2].min())   # the lowest offending edge
    out["shared_edge"] = (cells, f"nodes {first // nn} and {first % nn}")
    cells = ref.cell_nodes.copy()
    cells[20] = [4, 4, 7]
    out["repeated_node"] = (cells, "cell 20 ")
    for label, bad in (("index_nnodes", nn), ("index_negative", -1)):
        cells = ref.cell_nodes.copy()
        cells[17, 1] = bad
        cells[30, 2] = bad   # a second offender: the lowest cell is named
        out[label] = (cells, "cell 17 ")
    return out


@pytest.mark.parametrize("case", ["shared_edge", "repeated_node", "index_nnodes", "index_negative"])
@pytest.mark.parametrize("device", [False, True])
def test_malformed_cells_are_refused(case, device):
    """Ordinary error returns: the kernels form their keys from the bad values and never index with them."""
    import torch
    from dolfinx_eqlb_amd import cpp
    ref = reference("sq3")
    cells, text = _malformed()[case]
    L = cpp.lib()
    sentinel = 0x5EED5EED
    h = C.c_void_p(sentinel)
    if device:
        dx, dc = torch.from_numpy(ref.x).to("cuda"), torch.from_numpy(cells).to("cuda")
        torch.cuda.synchronize()
        px, pc = C.c_void_p(dx.data_ptr()), C.c_void_p(dc.data_ptr())
    else:
        hx = np.ascontiguousarray(ref.x)
        px, pc = hx.ctypes.data_as(C.c_void_p), cells.ctypes.data_as(C.c_void_p)
    st = L.eqlb_mesh_create_from_cells(C.c_int32(ref.nnodes), C.c_int32(ref.ncells), px, pc,
                                       C.c_int32(cpp.MEM_DEVICE if device else cpp.MEM_HOST), None, C.byref(h))
    msg = L.eqlb_last_error().decode()
    assert st == INVALID_ARGUMENT, (st, msg)
    assert "eqlb_mesh_create_from_cells" in msg and text in msg, msg
    assert h.value == sentinel
    with pytest.raises(RuntimeError, match="eqlb_mesh_create_from_cells"):
        cpp.DeviceMesh.from_cells(ref.x, cells)
    # the next valid call works
    if device:
        good = torch.from_numpy(ref.cell_nodes).to("cuda")
        assert_is(cpp.DeviceMesh.from_cells(dx, good, device=True), ref)
    else:
        assert_is(cpp.DeviceMesh.from_cells(ref.x, ref.cell_nodes), ref)


# ---- 8: the pybind carrier -------------------------------------------------------------------------------------------
def test_pybind_mesh_from_cells(oracle_mod):
    from dolfinx_eqlb_amd import _cpp as c
    from dolfinx_eqlb_amd.eqlb import _adapter as ad
    from cases import make_case
    k = 2
    mesh, ft, G, f = make_case(5, k, "neumann_lt")
    built = c.Mesh.from_cells(mesh.x[:, :2], mesh.cell_nodes)
    assert (built.nnodes, built.ncells, built.nfacets) == (mesh.nnodes, mesh.ncells, mesh.nfacets)
    assert built.max_patch_cells == ad.cpp_mesh(mesh).max_patch_cells
    assert np.array_equal(built.boundary_facets(), mesh.boundary_facets())
    assert np.array_equal(ad.cpp_mesh(mesh).boundary_facets(), mesh.boundary_facets())
    assert np.array_equal(built.find_facets(mesh.facet_nodes[:, ::-1]), np.arange(mesh.nfacets))
    assert np.array_equal(built.find_facets(np.array([[0, 0], [-1, 2]], dtype=np.int32)), [-1, -1])

    def run(m):
        V = c.FunctionSpace(m, "RT", k, 1, True)
        Vg, Vf = c.FunctionSpace(m, "DG", k - 1, 2, True), c.FunctionSpace(m, "DG", k - 1, 1, True)
        nq = c.facet_quadrature(c.interpolation_quadrature_degree(k))[0].size
        bcs = [[c.FluxBC(V, [int(i) for i in np.nonzero(ft[0] == 2)[0]], 0, nq, [], [], [])]]
        prime = [[int(i) for i in np.nonzero(ft[0] == 1)[0]]]
        bd = c.BoundaryData(bcs, [c.Function(V)], V, True, 2 * (k - 1), prime, False)
        flux = [c.Function(V)]
        c.reconstruct_fluxes_semiexplt(flux, [c.Function(Vg, G[0].copy())], [c.Function(Vf, f[0].copy())], bd, False)
        return flux[0].array.copy()

    a, b = run(ad.cpp_mesh(mesh)), run(built)
    assert np.array_equal(a, b)
    ref = oracle_mod.se_reconstruct(mesh, k, ft, G, f)[0]
    assert np.abs(b - ref).max() <= 1e-11 * np.abs(ref).max()
