"""Boundary conditions carried across a refinement on the device (eqlb_refine_facet_types, eqlb_refine_child_facets,
eqlb_refine_prolong_flux_bc, eqlb_se_carry_boundary / eqlb_ev_carry_boundary) against the numpy statement
dolfinx_eqlb_amd.mesh.refine.carry_facet_types / child_facets and mesh.transfer.prolong_flux_bc: types and children
bit for bit; values within 2 k eps A, the exact parts bit for bit; device memory on a caller's stream; the refusals;
against moments evaluated directly on the refined mesh; handles built by the carry against handles built through
set_boundary; the mirror classes.  Meshes of refine_cases only (at most 901 cells)."""

import ctypes as C
import functools

import numpy as np
import pytest

from refine_cases import NAMES, case

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
INVALID_ARGUMENT = -1
DEGREES, NRHS = (1, 2, 3, 4), (1, 3)


@pytest.fixture(scope="module")
def cpp():
    from dolfinx_eqlb_amd import cpp
    return cpp


def handle(cpp, mesh, created):
    return cpp.DeviceMesh(mesh) if created else cpp.DeviceMesh.from_cells(mesh.x, mesh.cell_nodes)


def facet_geometry(mesh, facets):
    cells = mesh.facet_cells[mesh.facet_cells_offsets[facets]]
    lf = np.argmax(mesh.cell_facets[cells] == np.asarray(facets)[:, None], axis=1)
    return cells, lf


def dense_table(mesh, k, dofs_by_row):
    """[nrhs, ncells*k(k+2)] from [(facets, dofs [nlist, k]) per row]: the array eqlb_se_set_boundary takes."""
    nrt = k * (k + 2)
    bv = np.zeros((len(dofs_by_row), mesh.ncells * nrt))
    for r, (facets, dofs) in enumerate(dofs_by_row):
        cells, lf = facet_geometry(mesh, facets)
        for j in range(k):
            bv[r, cells * nrt + lf * k + j] = dofs[:, j]
    return bv


def random_table(mesh, k, nrhs, rng):
    """Random DOFs on the boundary facets, zero elsewhere."""
    bf = mesh.boundary_facets()
    return dense_table(mesh, k, [(bf, rng.standard_normal((bf.size, k))) for _ in range(nrhs)])


def field(k, row=0):
    """A vector field of degree k - 1 with the callable signature of fluxbc / synthetic: its normal component on a
    straight facet is a polynomial of degree k - 1 in the facet parameter."""
    c = np.array([[0.7, 0.5, -0.2, 0.35, -0.45, 0.25, 0.3, -0.2, 0.15, 0.1],
                  [-0.4, 0.1, 0.6, -0.3, 0.2, 0.5, -0.25, 0.3, 0.1, -0.15]])
    if row:
        c = 0.8 * c[::-1] + 0.1
    monos = [(a, d - a) for d in range(k) for a in range(d, -1, -1)]

    def w(x, y):
        return tuple(sum(c[i, n] * x ** a * y ** b for n, (a, b) in enumerate(monos)) + 0.0 * x for i in (0, 1))
    return w


# -------------------------------------------------------------------------------------------- types and children
@pytest.mark.parametrize("created", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_types_and_children_equal_the_statement(cpp, name, created):
    from dolfinx_eqlb_amd.mesh import carry_facet_types, child_facets
    mesh, marked = case(name)
    dm = handle(cpp, mesh, created)
    r = dm.refine(marked, keep_plan=True)
    mesh2, pf, npf = r.dmesh.mesh, r.parent_facet, r.node_parent_facet
    rng = np.random.default_rng(21)
    bf = mesh.boundary_facets()
    for nrhs in NRHS:
        ft = np.zeros((nrhs, mesh.nfacets), dtype=np.int8)
        ft[:, bf] = rng.integers(1, 3, (nrhs, bf.size))
        got = r.facet_types(ft)
        assert got.dtype == np.int8 and got.shape == (nrhs, mesh2.nfacets)
        assert np.array_equal(got, carry_facet_types(ft, pf))
        assert np.array_equal(r.facet_types(ft[0]), got[0])
        ncell2 = np.diff(mesh2.facet_cells_offsets)
        assert np.all(got[:, ncell2 == 1] > 0) and np.all(got[:, ncell2 == 2] == 0)
    ft[0, bf[0]] = 9   # copied as it is
    assert np.array_equal(r.facet_types(ft), carry_facet_types(ft, pf))
    every = np.arange(mesh.nfacets, dtype=np.int32)
    ch = r.child_facets(every)
    assert ch.dtype == np.int32 and np.array_equal(ch, child_facets(mesh, npf, mesh2))
    pick = rng.integers(0, mesh.nfacets, 19).astype(np.int32)
    assert np.array_equal(r.child_facets(pick), ch[pick])
    flat = r.child_facets(bf, flat=True)
    assert np.array_equal(np.sort(flat), mesh2.boundary_facets())
    assert r.child_facets(np.zeros(0, dtype=np.int32)).shape == (0, 2)
    r.close()


# ------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("created", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_values_equal_the_statement(cpp, name, created):
    """|device - statement| <= 2 k eps A (both sides add k products of the same table entries: at most k eps/2 A each
    to first order; 2 is the margin); bit for bit on the whole, equally directed facets, at k = 1 and between two
    runs; a case with nothing marked returns the input."""
    from dolfinx_eqlb_amd.mesh import prolong_flux_bc
    from dolfinx_eqlb_amd.mesh.transfer import flux_bc_maps
    mesh, marked = case(name)
    dm = handle(cpp, mesh, created)
    r = dm.refine(marked, keep_plan=True)
    mesh2, pc, npf = r.dmesh.mesh, r.parent_cell, r.node_parent_facet
    bf2 = mesh2.boundary_facets().astype(np.int32)
    rng = np.random.default_rng(22)
    facets2 = rng.permutation(bf2)
    C2, l2, P, l, m = flux_bc_maps(mesh, mesh2, pc, npf, facets2)
    sigma = np.where(l2 == 1, 1.0, -1.0) * np.where(l == 1, 1.0, -1.0)
    worst = 0.0
    for k in DEGREES:
        nrt = k * (k + 2)
        for nrhs in NRHS:
            bv = random_table(mesh, k, nrhs, rng)
            got = r.prolong_flux_bc(k, bv, facets2)
            ref, A = prolong_flux_bc(mesh, mesh2, pc, npf, k, bv, facets2, return_abs=True)
            assert got.shape == ref.shape == (nrhs, facets2.size, k)
            err = np.abs(got - ref)
            assert np.all(A > 0)
            worst = max(worst, float((err / (EPS * A)).max()))
            assert np.all(err <= 2 * k * EPS * A), (k, nrhs)
            d = bv.reshape(nrhs, mesh.ncells, nrt)[:, P[:, None], l[:, None] * k + np.arange(k)[None, :]]
            whole = m == 0
            assert np.array_equal(got[:, whole], sigma[None, whole, None] * d[:, whole])
            if k == 1:
                assert np.array_equal(got, ref)
            assert np.array_equal(r.prolong_flux_bc(k, bv, facets2), got)          # two runs
            assert np.array_equal(r.prolong_flux_bc(k, bv[0], facets2), got[0])    # a single row
            if mesh2.ncells == mesh.ncells:                                        # nothing marked: the input
                assert np.array_equal(C2, P) and np.array_equal(l2, l) and np.array_equal(got, d)
    print(f"  {name}: max |err| / (eps A) = {worst:.2f} of 2 k")
    assert r.prolong_flux_bc(2, random_table(mesh, 2, 1, rng), np.zeros(0, dtype=np.int32)).shape == (1, 0, 2)
    r.close()


# ------------------------------------------------------------------------------------- device memory and refusals
def test_device_memory_on_a_non_blocking_stream(cpp):
    """Everything on a caller's non-blocking stream, the outputs between guard rows; in the device memory space a bad
    list entry gives a NaN row or (-1, -1) with its neighbours written."""
    import torch
    mesh, marked = case("lshape")
    dm = cpp.DeviceMesh.from_cells(mesh.x, mesh.cell_nodes)
    host = dm.refine(marked, keep_plan=True)
    mesh2 = host.dmesh.mesh
    nf, nf2 = mesh.nfacets, mesh2.nfacets
    rng = np.random.default_rng(23)
    k, nrhs = 3, 3
    bf, bf2 = mesh.boundary_facets().astype(np.int32), mesh2.boundary_facets().astype(np.int32)
    ft = np.zeros((nrhs, nf), dtype=np.int8)
    ft[:, bf] = rng.integers(1, 3, (nrhs, bf.size))
    bv = random_table(mesh, k, nrhs, rng)
    interior2 = int(np.nonzero(np.diff(mesh2.facet_cells_offsets) == 2)[0][5])
    no_parent = int(np.nonzero(np.asarray(host.parent_facet) < 0)[0][0])
    old_list = np.concatenate([bf[:7], [-1, nf, 2 ** 31 - 1, -2 ** 31], bf[7:]]).astype(np.int32)
    bad_old = np.isin(np.arange(old_list.size), [7, 8, 9, 10])
    new_list = np.concatenate([bf2[:5], [interior2, nf2, -3, no_parent, -2 ** 31], bf2[5:]]).astype(np.int32)
    bad_new = np.isin(np.arange(new_list.size), [5, 6, 7, 8, 9])
    want_ft, want_ch = host.facet_types(ft), host.child_facets(bf)
    want_dofs = host.prolong_flux_bc(k, bv, bf2)

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ids = torch.from_numpy(marked).to("cuda")
        count = torch.tensor([marked.size], dtype=torch.int64, device="cuda")
        r = dm.refine((ids, count), device=True, stream=stream.cuda_stream, keep_plan=True)
        d_ft, d_bv = torch.from_numpy(ft).to("cuda"), torch.from_numpy(bv).to("cuda")
        d_old, d_new = torch.from_numpy(old_list).to("cuda"), torch.from_numpy(new_list).to("cuda")
        g_ft = torch.full((3, nrhs * nf2), 77, dtype=torch.int8, device="cuda")
        g_ch = torch.full((3, 2 * old_list.size), -77, dtype=torch.int32, device="cuda")
        g_dofs = torch.full((3, nrhs * new_list.size * k), -7.25e300, dtype=torch.float64, device="cuda")
        r.plan.facet_types_raw(r.dmesh, nrhs, d_ft.data_ptr(), g_ft[1].data_ptr(), cpp.MEM_DEVICE, stream.cuda_stream)
        r.plan.child_facets_raw(r.dmesh, old_list.size, d_old.data_ptr(), g_ch[1].data_ptr(), cpp.MEM_DEVICE,
                                stream.cuda_stream)
        r.plan.prolong_flux_bc_raw(r.dmesh, k, nrhs, d_bv.data_ptr(), new_list.size, d_new.data_ptr(),
                                   g_dofs[1].data_ptr(), cpp.MEM_DEVICE, stream.cuda_stream)
        t_ft = r.facet_types(d_ft, stream=stream.cuda_stream)
        t_ch = r.child_facets(torch.from_numpy(bf).to("cuda"), stream=stream.cuda_stream)
        t_dofs = r.prolong_flux_bc(k, d_bv, torch.from_numpy(bf2).to("cuda"), stream=stream.cuda_stream)
    stream.synchronize()
    assert t_ft.is_cuda and t_ch.is_cuda and t_dofs.is_cuda
    assert np.array_equal(t_ft.cpu().numpy(), want_ft) and np.array_equal(t_ch.cpu().numpy(), want_ch)
    assert np.array_equal(t_dofs.cpu().numpy(), want_dofs)
    g = g_ft.cpu().numpy()
    assert np.all(g[0] == 77) and np.all(g[2] == 77) and np.array_equal(g[1].reshape(nrhs, nf2), want_ft)
    g = g_ch.cpu().numpy()
    assert np.all(g[0] == -77) and np.all(g[2] == -77)
    ch = g[1].reshape(-1, 2)
    assert np.all(ch[bad_old] == -1) and np.array_equal(ch[~bad_old], want_ch)
    g = g_dofs.cpu().numpy()
    assert np.all(g[0] == -7.25e300) and np.all(g[2] == -7.25e300)
    dofs = g[1].reshape(nrhs, new_list.size, k)
    assert np.all(np.isnan(dofs[:, bad_new])) and np.array_equal(dofs[:, ~bad_new], want_dofs)
    r.close()
    host.close()


def _raw(cpp, name, *args):
    L = cpp.lib()
    st = getattr(L, name)(*args)
    return int(st), L.eqlb_last_error().decode()


def test_refusals_each_followed_by_a_valid_call(cpp):
    mesh, marked = case("lshape")
    dm = cpp.DeviceMesh.from_cells(mesh.x, mesh.cell_nodes)
    r = dm.refine(marked, keep_plan=True)
    mesh2 = r.dmesh.mesh
    nf, nf2 = mesh.nfacets, mesh2.nfacets
    k = 2
    rng = np.random.default_rng(24)
    bf, bf2 = mesh.boundary_facets().astype(np.int32), mesh2.boundary_facets().astype(np.int32)
    ft = np.zeros((1, nf), dtype=np.int8)
    ft[:, bf] = 1
    bv = random_table(mesh, k, 1, rng)
    good = (r.facet_types(ft), r.child_facets(bf), r.prolong_flux_bc(k, bv, bf2))

    def valid():
        now = (r.facet_types(ft), r.child_facets(bf), r.prolong_flux_bc(k, bv, bf2))
        assert all(np.array_equal(a, b) for a, b in zip(now, good))

    ft2 = np.full((1, nf2), 77, dtype=np.int8)
    ch = np.full((bf.size + 1, 2), -77, dtype=np.int32)
    dofs = np.full((1, bf2.size + 1, k), -7.25e300)
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    i32 = C.c_int32
    plan, fine, coarse = r.plan._h, r.dmesh._h, dm._h

    def types(plan=plan, refined=fine, nrhs=1, memspace=0):
        return _raw(cpp, "eqlb_refine_facet_types", plan, refined, i32(nrhs), p(ft), p(ft2), i32(memspace), None)

    def children(plan=plan, refined=fine, nlist=bf.size, memspace=0, facets=bf):
        return _raw(cpp, "eqlb_refine_child_facets", plan, refined, i32(nlist), p(facets), p(ch), i32(memspace), None)

    def values(plan=plan, refined=fine, k=k, nrhs=1, nlist=bf2.size, memspace=0, facets2=bf2):
        return _raw(cpp, "eqlb_refine_prolong_flux_bc", plan, refined, i32(k), i32(nrhs), p(bv), i32(nlist),
                    p(facets2), p(dofs), i32(memspace), None)

    for call, entry, cases in ((types, "eqlb_refine_facet_types", (dict(refined=coarse), dict(nrhs=0),
                                                                   dict(memspace=2))),
                               (children, "eqlb_refine_child_facets", (dict(refined=coarse), dict(nlist=-1),
                                                                       dict(memspace=2))),
                               (values, "eqlb_refine_prolong_flux_bc", (dict(refined=coarse), dict(k=0), dict(k=5),
                                                                        dict(nrhs=0), dict(nlist=-1),
                                                                        dict(memspace=2)))):
        for kw in cases:
            st, msg = call(**kw)
            assert st == INVALID_ARGUMENT and entry in msg, (kw, msg)
            if "refined" in kw:
                assert "refined mesh" in msg, msg
            valid()
    # host memory: the offender by name, nothing written
    for bad in (nf, -1):
        st, msg = children(nlist=bf.size + 1, facets=np.append(bf, bad).astype(np.int32))
        assert st == INVALID_ARGUMENT and "facets[%d] = %d is no facet of the mesh" % (bf.size, bad) in msg, msg
    interior2 = int(np.nonzero(np.diff(mesh2.facet_cells_offsets) == 2)[0][0])
    for bad, words in ((nf2, "is no facet of the refined mesh"), (-1, "is no facet of the refined mesh"),
                       (interior2, "lies between two cells")):
        st, msg = values(nlist=bf2.size + 1, facets2=np.append(bf2, bad).astype(np.int32))
        assert st == INVALID_ARGUMENT and "facets2[%d] = %d %s" % (bf2.size, bad, words) in msg, msg
    with pytest.raises(RuntimeError, match="lies between two cells"):
        r.prolong_flux_bc(k, bv, [interior2])
    assert np.all(ft2 == 77) and np.all(ch == -77) and np.all(dofs == -7.25e300)
    valid()
    # and the raw entries write what the wrappers return
    assert types()[0] == 0 and children()[0] == 0 and values()[0] == 0
    assert np.array_equal(ft2, good[0]) and np.array_equal(ch[:-1], good[1]) and np.all(ch[-1] == -77)
    assert np.array_equal(dofs.reshape(-1)[:bf2.size * k], good[2].reshape(-1))
    r.close()
    with pytest.raises(RuntimeError, match="keep_plan"):
        r.child_facets(bf)


# ------------------------------------------------------------------------------------ against direct evaluation
@pytest.mark.parametrize("name", ["lshape", "hole"])
@pytest.mark.parametrize("k", DEGREES)
def test_carried_dofs_against_moments_on_the_refined_mesh(cpp, name, k):
    """A normal flux g = p(x, y), p of total degree k - 1 (a polynomial of degree k - 1 in the parameter of every
    facet), with a k-point Gauss rule (exact to degree 2k - 1): eqlb_flux_bc_dofs on the coarse handle, carried,
    against eqlb_flux_bc_dofs on the refined handle.

    Bound, as in tests/test_bc_carry_host.py, in units of eps, with M = sum |c_ab| R^(a+b) >= |g| and
    R = max(1, max |x|):
      a point value: 2k roundings of the evaluation (k eps M); the points of eqlb_facet_points are off by at most
      8 eps R (tests/test_gpu_bc_update.py) and the midpoints of the refinement by eps/2 R, which moves p by at most
      (k - 1) M / R per unit in either coordinate: 2 (k - 1) 9 eps M.  Together at most 19 k eps M;
      a DOF = scale sum_q (w_q g_q) s_q^j: at most 2k + 2 roundings ((k + 1) eps), the rounded rule (k eps), the
      scale |E| from rounded differences, a sum of squares and a root (2 eps): N = 22 k + 3 against |E| M;
      on the refined mesh the ends of a facet are off by eps/2 R each, which changes its length by at most
      2 eps R: N2 = N + 2 R / |E2|;
      the carry: the errors of the parent DOFs through |FB|, k + 1 roundings (eps / 2 each) against
      A_j <= sum_i |FB_ji| |E| M.
    |carried - direct| <= 2 eps M (|E| (N + (k + 1) / 2) sum_i |FB_ji| + |E2| N2), 2 the margin."""
    from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_interval
    from dolfinx_eqlb_amd.mesh import flux_bc_table
    from dolfinx_eqlb_amd.mesh.transfer import flux_bc_maps
    mesh, marked = case(name)
    dm = cpp.DeviceMesh.from_cells(mesh.x, mesh.cell_nodes)
    r = dm.refine(marked, keep_plan=True)
    mesh2 = r.dmesh.mesh
    s, wq = make_quadrature_interval(2 * k - 1)
    assert s.size == k
    rng = np.random.default_rng(30 + k)
    monos = [(a, d - a) for d in range(k) for a in range(d, -1, -1)]
    coef = rng.standard_normal(len(monos))

    def g(x, y):
        return sum(c * x ** a * y ** b for c, (a, b) in zip(coef, monos)) + 0.0 * x

    def dofs_on(handle_, m_, facets):
        xq = cpp.facet_points(handle_, facets, s)
        return cpp.flux_bc_dofs(handle_, k, facets, s, wq, g(xq[..., 0], xq[..., 1]))

    bf, bf2 = mesh.boundary_facets().astype(np.int32), mesh2.boundary_facets().astype(np.int32)
    table = dense_table(mesh, k, [(bf, dofs_on(dm, mesh, bf))])
    carried = r.prolong_flux_bc(k, table, bf2)[0]
    direct = dofs_on(r.dmesh, mesh2, bf2)
    C2, l2, P, l, m = flux_bc_maps(mesh, mesh2, r.parent_cell, r.node_parent_facet, bf2)
    assert np.count_nonzero(np.bincount(m, minlength=6)) >= 4
    R = max(1.0, float(np.abs(mesh2.x).max()))
    M = float(sum(abs(c) * R ** (a + b) for c, (a, b) in zip(coef, monos)))
    e2 = mesh2.x[mesh2.facet_nodes[bf2, 1], :2] - mesh2.x[mesh2.facet_nodes[bf2, 0], :2]
    E2 = np.hypot(e2[:, 0], e2[:, 1])
    E = np.where(m >= 2, 2.0, 1.0) * E2
    N = 22 * k + 3
    FBabs = np.abs(flux_bc_table(k))[m].sum(axis=2)                               # [n, k]
    bound = 2 * EPS * M * (E[:, None] * (N + 0.5 * (k + 1)) * FBabs + (E2 * (N + 2 * R / E2))[:, None])
    err = np.abs(carried - direct)
    print(f"  {name} k = {k}: worst |carried - direct| / bound = {(err / bound).max():.3f}, "
          f"/ max|dof| = {err.max() / np.abs(direct).max():.2e}")
    assert np.abs(direct).max() > 1e-3 and np.all(err <= bound)
    r.close()


# ------------------------------------------------------------------------------------------------------ handles
@functools.lru_cache(maxsize=None)
def layout(name):
    """(mesh, marked, ft [1, nfacets]): `lshape` with flux conditions on the sides x = 0 and y = 0 and Dirichlet
    elsewhere, `hole` with the pure flux-BC loop round the hole."""
    from synthetic import facet_types
    mesh, marked = case(name)
    if name == "hole":
        from topology_meshes import facet_table
        ft = facet_table(mesh, "flux_middle")
    else:
        ft = facet_types(mesh, lambda p: (p[:, 0] < 1e-9) | (p[:, 1] < 1e-9))
    assert (ft[0] == 2).any() and (ft[0] == 1).any()
    return mesh, marked, ft


def two_routes(cpp, make, old, r, ft, k):
    """`fresh` built by the carry and by set_boundary with the dense table scattered from the output of
    eqlb_refine_prolong_flux_bc: (carried handle, other handle, ft2, table2 or None)."""
    mesh2 = r.dmesh.mesh
    nrhs = ft.shape[0]
    a = make(r.dmesh)
    a.carry_boundary(old, r)
    ft2 = r.facet_types(ft)
    bv = old.get_boundary_values()
    table2 = None
    if bv.any():
        rows = []
        for q in range(nrhs):
            f2 = np.nonzero(ft2[q] == 2)[0].astype(np.int32)
            rows.append((f2, r.prolong_flux_bc(k, bv[q], f2)))
        table2 = dense_table(mesh2, k, rows)
    b = make(r.dmesh)
    b.set_boundary(ft2, boundary_values=table2)
    ta, tb = a.get_boundary_values(), b.get_boundary_values()
    assert np.array_equal(ta, tb)
    if table2 is not None:
        assert np.array_equal(ta, table2) and np.abs(ta).max() > 0
    else:
        assert not ta.any()
    return a, b, ft2, table2


def se_maker(cpp, k, nrhs, stress=False):
    def make(dmesh):
        eq = cpp.SemiExplicitEquilibrator(dmesh, k, nrhs, reconstruct_stress=stress)
        eq.set_option("accumulate", 0)
        return eq
    return make


@pytest.mark.parametrize("name,k", [("lshape", 2), ("lshape", 3), ("hole", 2)])
def test_se_handle_by_carry_equals_handle_by_set_boundary(cpp, name, k):
    """Tables and one sweep bit for bit, with the coarse data prolonged by eqlb_refine_prolong_dg and with data that
    are compatible on the refined mesh with the carried condition (the coarse data are not: their orthogonality
    holds against the coarse hat functions only); with the latter the facet DOFs of the flux meet the carried table
    within the bound of tests/test_gpu_bc_update.py.  Then a second level, the carried handle as `old`; and an `old`
    without a table."""
    from synthetic import boundary_dofs_from_field, make_compatible_data
    mesh, marked, ft = layout(name)
    w = field(k)
    d = k - 1
    G, f = make_compatible_data(mesh, k, ft, neumann_flux=w, seed=41)
    dm = cpp.DeviceMesh.from_cells(mesh.x, mesh.cell_nodes)
    make = se_maker(cpp, k, 1)
    old = make(dm)
    old.set_boundary(ft, boundary_values=boundary_dofs_from_field(mesh, k, ft[0], w)[None])
    r = dm.refine(marked, keep_plan=True)
    mesh2 = r.dmesh.mesh
    a, b, ft2, table2 = two_routes(cpp, make, old, r, ft, k)
    facets2 = np.nonzero(ft2[0] == 2)[0].astype(np.int32)
    assert facets2.size > np.count_nonzero(ft[0] == 2)
    # the carried table is the condition itself on the refined mesh
    direct = boundary_dofs_from_field(mesh2, k, ft2[0], w)
    assert np.abs(table2[0] - direct).max() <= 1e-12 * np.abs(direct).max()
    G2p, f2p = r.prolong_dg(d, G[None], bs=2), r.prolong_dg(d, f[None])
    xa, xb = a.equilibrate_host(G2p, f2p), b.equilibrate_host(G2p, f2p)
    assert np.isfinite(xa).all() and np.abs(xa).max() > 0 and np.array_equal(xa, xb)
    G2, f2 = make_compatible_data(mesh2, k, ft2, neumann_flux=w, seed=42)
    xa, xb = a.equilibrate_host(G2[None], f2[None]), b.equilibrate_host(G2[None], f2[None])
    assert np.array_equal(xa, xb)
    res = cpp.boundary_residual(r.dmesh, k, xa, G2[None], facets2, boundary_values=a.get_boundary_values())
    print(f"  {name} k = {k}: boundary residual / max|bv| = {res.max() / np.abs(table2).max():.2e}")
    assert res.max() <= 1e-11 * np.abs(table2).max()

    # second level: the handle of level 1 is `old`
    marks2 = np.arange(0, mesh2.ncells, 5, dtype=np.int32)
    r2 = r.dmesh.refine(marks2, keep_plan=True)
    a2, b2, ft3, table3 = two_routes(cpp, make, a, r2, ft2, k)
    mesh3 = r2.dmesh.mesh
    direct3 = boundary_dofs_from_field(mesh3, k, ft3[0], w)
    assert np.abs(table3[0] - direct3).max() <= 1e-12 * np.abs(direct3).max()
    G3, f3 = make_compatible_data(mesh3, k, ft3, neumann_flux=w, seed=43)
    x3 = a2.equilibrate_host(G3[None], f3[None])
    assert np.array_equal(x3, b2.equilibrate_host(G3[None], f3[None]))
    facets3 = np.nonzero(ft3[0] == 2)[0].astype(np.int32)
    res = cpp.boundary_residual(r2.dmesh, k, x3, G3[None], facets3, boundary_values=table3)
    assert res.max() <= 1e-11 * np.abs(table3).max()
    r2.close()

    # an old handle without a table leaves the new one without a table
    plain = make(dm)
    plain.set_boundary(ft)
    a0, b0, _, none = two_routes(cpp, make, plain, r, ft, k)
    assert none is None
    G0, f0 = make_compatible_data(mesh2, k, ft2, seed=44)
    assert np.array_equal(a0.equilibrate_host(G0[None], f0[None]), b0.equilibrate_host(G0[None], f0[None]))
    # a node mask goes to the planner as set_boundary takes it
    mask = (np.arange(mesh2.nnodes) % 3 != 0).astype(np.uint8)
    am, bm = make(r.dmesh), make(r.dmesh)
    am.carry_boundary(old, r, node_mask=mask)
    bm.set_boundary(ft2, boundary_values=table2, node_mask=mask)
    assert am.num_patches == bm.num_patches < a.num_patches
    assert np.array_equal(am.equilibrate_host(G2[None], f2[None]), bm.equilibrate_host(G2[None], f2[None]))
    r.close()


def test_stress_handle_with_tractions_on_both_rows(cpp):
    from synthetic import boundary_dofs_from_field, make_compatible_stress_data
    k = 2
    mesh, marked, ft1 = layout("lshape")
    ft = np.repeat(ft1, 2, axis=0)
    ws = [field(k, 0), field(k, 1)]
    dm = cpp.DeviceMesh.from_cells(mesh.x, mesh.cell_nodes)
    make = se_maker(cpp, k, 2, stress=True)
    old = make(dm)
    old.set_boundary(ft, boundary_values=np.stack([boundary_dofs_from_field(mesh, k, ft[q], ws[q]) for q in (0, 1)]))
    r = dm.refine(marked, keep_plan=True)
    mesh2 = r.dmesh.mesh
    a, b, ft2, table2 = two_routes(cpp, make, old, r, ft, k)
    assert np.abs(table2[0]).max() > 0 and np.abs(table2[1]).max() > 0 and not np.array_equal(table2[0], table2[1])
    G2, f2 = make_compatible_stress_data(mesh2, k, ft2, neumann_flux=ws, seed=45)
    xa, xb = a.equilibrate_host(G2, f2), b.equilibrate_host(G2, f2)
    assert np.isfinite(xa).all() and np.array_equal(xa, xb)
    facets2 = np.nonzero(ft2[0] == 2)[0].astype(np.int32)
    res = cpp.boundary_residual(r.dmesh, k, xa, G2, facets2, boundary_values=a.get_boundary_values())
    assert res.shape == (2, facets2.size) and res.max() <= 1e-11 * np.abs(table2).max()
    r.close()


def test_ev_handle_by_carry(cpp):
    """eqlb_ev_carry_boundary at k = 2 on the broken per-cell table: bit for bit against a handle that got the output
    of eqlb_refine_prolong_flux_bc through eqlb_ev_update_flux_bc (the same DOFs written into the same table), and
    within the tolerance of tests/test_gpu_bc_update.py against one that got them as conforming values through
    eqlb_ev_set_boundary, which converts them."""
    from dolfinx_eqlb_amd.eqlb.conforming import broken_to_conforming
    from synthetic import boundary_dofs_from_field, make_compatible_data
    k = 2
    mesh, marked, ft = layout("lshape")
    w = field(k)
    dm = cpp.DeviceMesh.from_cells(mesh.x, mesh.cell_nodes)

    def make(dmesh):
        ev = cpp.ConstrainedMinEquilibrator(dmesh, k, 1)
        ev.set_option("output", 1)
        return ev

    bv = boundary_dofs_from_field(mesh, k, ft[0], w)
    old = make(dm)
    old.set_boundary(ft, boundary_values=broken_to_conforming(mesh, k, bv)[None])
    r = dm.refine(marked, keep_plan=True)
    mesh2 = r.dmesh.mesh
    a = make(r.dmesh)
    a.carry_boundary(old, r)
    ft2 = r.facet_types(ft)
    facets2 = np.nonzero(ft2[0] == 2)[0].astype(np.int32)
    dofs = r.prolong_flux_bc(k, old.get_boundary_values(), facets2)
    b = make(r.dmesh)
    b.set_boundary(ft2)
    b.update_flux_bc(0, facets2, dofs[0])
    ta = a.get_boundary_values()
    assert np.abs(ta).max() > 0 and np.array_equal(ta, b.get_boundary_values())
    assert np.array_equal(ta, dense_table(mesh2, k, [(facets2, dofs[0])]))
    G2, f2 = make_compatible_data(mesh2, k, ft2, neumann_flux=w, seed=46)
    xa, xb = a.equilibrate_host(G2[None], f2[None]), b.equilibrate_host(G2[None], f2[None])
    assert np.isfinite(xa).all() and np.array_equal(xa, xb)
    # the broken output is the total flux: its facet DOFs are the table
    res = cpp.boundary_residual(r.dmesh, k, xa, None, facets2, boundary_values=ta)
    assert res.max() <= 1e-11 * np.abs(ta).max()
    c = make(r.dmesh)
    c.set_boundary(ft2, boundary_values=broken_to_conforming(mesh2, k, ta[0])[None])
    xc = c.equilibrate_host(G2[None], f2[None])
    assert np.abs(xa - xc).max() <= 1e-11 * np.abs(xc).max()
    # without a table
    plain = make(dm)
    plain.set_boundary(ft)
    a0 = make(r.dmesh)
    a0.carry_boundary(plain, r)
    assert not a0.get_boundary_values().any()
    r.close()


def test_refusals_of_the_carry(cpp):
    """`old` without boundary data, another k, nrhs or stress flag, an `old` on another mesh, a `fresh` on the wrong
    mesh, a plan that is closed: after each, `fresh` still accepts a plain set_boundary and equilibrates."""
    from synthetic import make_compatible_data
    k = 2
    mesh, marked, ft = layout("lshape")
    dm = cpp.DeviceMesh.from_cells(mesh.x, mesh.cell_nodes)
    r = dm.refine(marked, keep_plan=True)
    mesh2 = r.dmesh.mesh
    ft2 = r.facet_types(ft)
    G2, f2 = make_compatible_data(mesh2, k, ft2, seed=47)
    old = cpp.SemiExplicitEquilibrator(dm, k, 1)
    old.set_boundary(ft)
    fresh = cpp.SemiExplicitEquilibrator(r.dmesh, k, 1)
    fresh.set_option("accumulate", 0)
    ref = cpp.SemiExplicitEquilibrator(r.dmesh, k, 1)
    ref.set_option("accumulate", 0)
    ref.set_boundary(ft2)
    want = ref.equilibrate_host(G2[None], f2[None])

    def still_works():
        fresh.set_boundary(ft2)
        assert np.array_equal(fresh.equilibrate_host(G2[None], f2[None]), want)

    unset = cpp.SemiExplicitEquilibrator(dm, k, 1)
    other_k = cpp.SemiExplicitEquilibrator(dm, 3, 1)
    other_k.set_boundary(ft)
    other_n = cpp.SemiExplicitEquilibrator(dm, k, 2)
    other_n.set_boundary(np.repeat(ft, 2, axis=0))
    stress = cpp.SemiExplicitEquilibrator(dm, k, 2, reconstruct_stress=True)
    stress.set_boundary(np.repeat(ft, 2, axis=0))
    elsewhere = cpp.SemiExplicitEquilibrator(r.dmesh, k, 1)
    elsewhere.set_boundary(ft2)
    for bad_old, words in ((unset, "no boundary data"), (other_k, "k = 3 and 2"), (other_n, "nrhs = 2 and 1"),
                           (elsewhere, "not the mesh of the plan")):
        with pytest.raises(RuntimeError, match="eqlb_se_carry_boundary.*" + words):
            fresh.carry_boundary(bad_old, r)
        still_works()
    fresh2 = cpp.SemiExplicitEquilibrator(r.dmesh, k, 2)
    with pytest.raises(RuntimeError, match="stress = 1 and 0"):
        fresh2.carry_boundary(stress, r)
    on_coarse = cpp.SemiExplicitEquilibrator(dm, k, 1)
    with pytest.raises(RuntimeError, match="eqlb_se_carry_boundary.*refined mesh"):
        on_coarse.carry_boundary(old, r)
    on_coarse.set_boundary(ft)
    with pytest.raises(RuntimeError, match="Input sizes"):
        fresh.carry_boundary(old, r, node_mask=np.ones(mesh.nnodes, dtype=np.uint8))
    L = cpp.lib()
    ev_old, ev_fresh = cpp.ConstrainedMinEquilibrator(dm, k, 1), cpp.ConstrainedMinEquilibrator(r.dmesh, k, 1)
    with pytest.raises(RuntimeError, match="eqlb_ev_carry_boundary.*no boundary data"):
        ev_fresh.carry_boundary(ev_old, r)
    assert L.eqlb_ev_carry_boundary(None, r.plan._h, ev_fresh._h, None, None) == INVALID_ARGUMENT
    ev_fresh.set_boundary(ft2)
    assert np.isfinite(ev_fresh.equilibrate_host(G2[None], f2[None])).all()
    fresh.carry_boundary(old, r)                       # the next valid call works
    assert np.array_equal(fresh.equilibrate_host(G2[None], f2[None]), want)
    r.close()
    with pytest.raises(RuntimeError, match="keep_plan"):
        fresh.carry_boundary(old, r)
    still_works()


# ------------------------------------------------------------------------------------------------------- mirror
def test_mirror_refined_and_the_pybind_carrier(cpp):
    """FluxEqlbSE.refined on `lshape` with one fluxbc callable.  The data are polynomials - u = a quadratic,
    G = -grad u in DG_1^2, f = div G - so that what eqlb_refine_prolong_dg carries over is compatible on the refined
    mesh as well (the Galerkin orthogonality of an exact solution holds on every mesh), with the flux G . n on the
    flux boundary."""
    from dolfinx_eqlb_amd import _cpp as c
    from dolfinx_eqlb_amd.eqlb import check_eqlb_conditions as chk
    from dolfinx_eqlb_amd.eqlb.FluxEqlbEV import FluxEqlbEV
    from dolfinx_eqlb_amd.eqlb.FluxEqlbSE import FluxEqlbSE, fluxbc
    from synthetic import boundary_dofs_from_field, dg_points
    k = 2
    mesh, marked, ft = layout("lshape")

    def flux(x, y):      # -grad(0.3 x^2 - 0.2 x y + 0.5 y^2 + 0.1 x - 0.4 y)
        return -(0.6 * x - 0.2 * y + 0.1), -(-0.2 * x + 1.0 * y - 0.4)

    pts = dg_points(mesh, 1)
    G = np.stack(flux(pts[..., 0], pts[..., 1]), axis=2).reshape(-1)
    f = np.full(mesh.ncells * 3, -1.6)
    prime, dual = np.nonzero(ft[0] == 1)[0].astype(np.int32), np.nonzero(ft[0] == 2)[0].astype(np.int32)

    dm = cpp.DeviceMesh.from_cells(mesh.x, mesh.cell_nodes)
    r = dm.refine(marked, keep_plan=True)
    base = c.Mesh.from_cells(mesh.x[:, :2], mesh.cell_nodes)
    new, parent_cell, node_parent_facet, parent_facet, tr = base.refine(marked, keep_plan=True)
    # the pybind carrier equals the ctypes route
    rng = np.random.default_rng(48)
    types = np.zeros((2, mesh.nfacets), dtype=np.int8)
    types[:, mesh.boundary_facets()] = rng.integers(1, 3, (2, mesh.boundary_facets().size))
    assert np.array_equal(tr.facet_types(types), r.facet_types(types))
    every = np.arange(mesh.nfacets, dtype=np.int32)
    assert np.array_equal(tr.child_facets(every), r.child_facets(every))
    bf2 = r.dmesh.mesh.boundary_facets().astype(np.int32)
    for kk in DEGREES:
        bv = random_table(mesh, kk, 2, rng)
        assert np.array_equal(tr.prolong_flux_bc(kk, bv, bf2), r.prolong_flux_bc(kk, bv, bf2))
    with pytest.raises(RuntimeError, match="lies between two cells"):
        tr.prolong_flux_bc(1, random_table(mesh, 1, 1, rng), np.setdiff1d(np.arange(new.nfacets), bf2)[:1])

    eq = FluxEqlbSE(k, mesh, [f], [G])
    with pytest.raises(RuntimeError, match="Boundary conditions have not been set"):
        eq.refined(tr, [f], [G])
    eq.set_boundary_conditions([prime], [[fluxbc(flux, dual)]])
    G2, f2 = tr.prolong_dg(1, G, bs=2)[0], tr.prolong_dg(1, f)[0]
    for carrier in (tr, r):
        eq2 = eq.refined(carrier, [f2], [G2])
        mesh2 = eq2.mesh
        assert mesh2.ncells == new.ncells and eq2.degree_flux == k
        prime2, dual2 = r.child_facets(prime, flat=True), r.child_facets(dual, flat=True)
        assert np.array_equal(eq2.list_bfct_prime[0], prime2)
        assert np.array_equal(eq2.list_bcs_flux[0][0].facets, dual2)
        assert np.array_equal(eq2.facet_type, r.facet_types(ft))
        eq2.equilibrate_fluxes()
        x = eq2.list_flux[0]
        assert np.isfinite(x).all()
        bv2 = boundary_dofs_from_field(mesh2, k, eq2.facet_type[0], flux)
        assert np.abs(bv2).max() > 1e-3
        assert np.abs(eq2.list_bfunctions[0] - bv2).max() <= 1e-12 * np.abs(bv2).max()
        assert chk.boundary_flux_residual(mesh2, k, x, G2, dual2, boundary_values=bv2) <= 1e-10
        res, nrm = chk.divergence_residual(mesh2, k, x, G2, f2)
        assert res <= 1e-10 * max(nrm, 1.0)
        assert chk.jump_residual(mesh2, k, x, G2) <= 1e-9
    ev = FluxEqlbEV(k, mesh, [f], [G])
    with pytest.raises(RuntimeError, match="Boundary conditions have not been set"):
        ev.refined(tr, [f2], [G2])
    ev.set_boundary_conditions([prime], [[fluxbc(flux, dual)]])
    ev2 = ev.refined(tr, [f2], [G2])
    assert np.array_equal(ev2.facet_type, r.facet_types(ft))
    ev2.equilibrate_fluxes()
    assert np.isfinite(ev2.list_flux).all()
    r.close()
