"""The statement of the refinement rule (dolfinx_eqlb_amd.mesh.refine) on the inputs of tests/refine_cases.py:
closure, conformity, areas, boundary and the parent tables."""

import numpy as np
import pytest

from refine_cases import NAMES, case, level_marks, sq40

_OUT = {}


def refined(name):
    if name not in _OUT:
        from dolfinx_eqlb_amd.mesh import create_mesh, parent_facets, refine_longest_edge
        mesh, marked = case(name)
        x2, c2, pc, npf = refine_longest_edge(mesh, marked)
        mesh2 = create_mesh(x2, c2)
        _OUT[name] = (x2, c2, pc, npf, mesh2, parent_facets(mesh, npf, mesh2))
    return _OUT[name]


def closure_by_doubling(mesh, marked):
    """Reachability along succ by pointer doubling, ceil(log2(ncells)) passes; returns (E, passes)."""
    from dolfinx_eqlb_amd.mesh.refine import longest_facets
    _, L = longest_facets(mesh)
    nc = mesh.ncells
    fo = mesh.facet_cells_offsets
    first, last = mesh.facet_cells[fo[L]], mesh.facet_cells[fo[L + 1] - 1]
    cells = np.arange(nc)
    succ = np.where(first == cells, last, first)       # the other cell of L(c), c itself on the boundary
    E = np.zeros(mesh.nfacets, dtype=bool)
    E[mesh.cell_facets[marked].ravel()] = True
    act = E[mesh.cell_facets].any(axis=1)
    jump = succ.copy()
    passes = int(np.ceil(np.log2(nc))) if nc > 1 else 0
    for _ in range(passes):
        act[jump[act]] = True
        jump = jump[jump]
    E[L[act]] = True
    return E, passes


def _area2(x, cells):
    p0, p1, p2 = x[cells[:, 0]], x[cells[:, 1]], x[cells[:, 2]]
    return (p1[:, 0] - p0[:, 0]) * (p2[:, 1] - p0[:, 1]) - (p1[:, 1] - p0[:, 1]) * (p2[:, 0] - p0[:, 0])


def _boundary_length(mesh):
    fn = mesh.facet_nodes[mesh.boundary_facets()]
    return np.sort(np.linalg.norm(mesh.x[fn[:, 0]] - mesh.x[fn[:, 1]], axis=1)).sum()


@pytest.mark.parametrize("name", NAMES)
def test_closure_by_sweeping_equals_doubling(name):
    from dolfinx_eqlb_amd.mesh.refine import closure_by_sweeping, longest_facets
    mesh, marked = case(name)
    E, sweeps = closure_by_sweeping(mesh, marked, return_passes=True)
    D, passes = closure_by_doubling(mesh, marked)
    assert np.array_equal(E, D)
    _, L = longest_facets(mesh)
    touched = E[mesh.cell_facets].any(axis=1)
    assert np.all(E[L[touched]])
    assert np.all(E[mesh.cell_facets[marked].ravel()])
    if name == "graded_first":
        assert passes == 9 and sweeps >= 299 and E.sum() == 302


@pytest.mark.parametrize("name", NAMES)
def test_refined_mesh_is_conforming_and_keeps_the_domain(name):
    mesh, marked = case(name)
    x2, c2, pc, npf, mesh2, _ = refined(name)
    assert c2.dtype == np.int32 and pc.dtype == np.int32 and npf.dtype == np.int32
    assert x2.shape == (mesh.nnodes + npf.size, 3) and np.array_equal(x2[:mesh.nnodes], mesh.x)
    assert np.diff(mesh2.facet_cells_offsets).max() <= 2
    assert np.array_equal(np.unique(c2), np.arange(x2.shape[0])) or mesh.nnodes > np.unique(mesh.cell_nodes).size
    # no hanging node: a bisected old edge is no edge of the new mesh
    nn2 = x2.shape[0]
    key2 = mesh2.facet_nodes[:, 0].astype(np.int64) * nn2 + mesh2.facet_nodes[:, 1]
    old = mesh.facet_nodes[npf].astype(np.int64)
    assert not np.isin(old.min(axis=1) * nn2 + old.max(axis=1), key2).any()
    # areas
    a_old, a_new = _area2(mesh.x, mesh.cell_nodes), _area2(x2, c2)
    assert np.all(np.sign(a_new) == np.sign(a_old)[pc]) and np.all(a_new != 0)
    sums = np.bincount(pc, weights=a_new, minlength=mesh.ncells)
    assert np.allclose(sums, a_old, rtol=1e-12, atol=0)
    assert np.isclose(_boundary_length(mesh2), _boundary_length(mesh), rtol=1e-12, atol=0)
    # parents
    assert np.all(np.diff(pc) >= 0)
    nch = np.bincount(pc, minlength=mesh.ncells)
    assert nch.min() >= 1 and nch.max() <= 4 and nch.sum() == c2.shape[0]
    if marked.size:
        assert np.all(nch[marked] == 4)
    else:
        assert np.array_equal(c2, mesh.cell_nodes) and npf.size == 0


@pytest.mark.parametrize("name", NAMES)
def test_parent_facets(name):
    mesh, _ = case(name)
    x2, c2, pc, npf, mesh2, pf = refined(name)
    assert pf.dtype == np.int32 and pf.shape == (mesh2.nfacets,)
    old_boundary = np.zeros(mesh.nfacets, dtype=bool)
    old_boundary[mesh.boundary_facets()] = True
    b2 = mesh2.boundary_facets()
    assert np.all(pf[b2] >= 0) and np.all(old_boundary[pf[b2]])
    # a facet with a parent lies on it: both nodes are ends or the midpoint of the parent
    has = np.nonzero(pf >= 0)[0]
    mid = np.full(mesh.nfacets, -1, dtype=np.int64)
    mid[npf] = mesh.nnodes + np.arange(npf.size)
    allowed = np.concatenate([mesh.facet_nodes[pf[has]], mid[pf[has]][:, None]], axis=1)
    for j in (0, 1):
        assert np.all((mesh2.facet_nodes[has, j][:, None] == allowed).any(axis=1))
    # every old facet is covered: once if unbisected, twice if bisected
    cover = np.bincount(pf[has], minlength=mesh.nfacets)
    want = np.ones(mesh.nfacets, dtype=np.int64)
    want[npf] = 2
    assert np.array_equal(cover, want)


def test_counts_of_the_strips():
    """(bisected facets, cells, cells cut): the graded strip propagates from cell 0 through all 300 cells and from
    cell 299 to its neighbour only; with ties the lower facet id decides, so cell 69 reaches all 70 cells."""
    want = {"graded_first": (302, 901, 300), "graded_last": (3, 304, 2), "ties_last": (72, 211, 70),
            "ties_first": (3, 74, 2), "right1": (3, 6, 2), "triangle": (3, 4, 1), "sq3_empty": (0, 36, 0)}
    for name, counts in want.items():
        x2, c2, pc, npf, _, _ = refined(name)
        assert (npf.size, c2.shape[0], int((np.bincount(pc) > 1).sum())) == counts, name
    assert np.array_equal(np.bincount(refined("right1")[2]), [4, 2])


def test_four_levels_on_the_perturbed_square():
    from dolfinx_eqlb_amd.mesh import create_mesh, refine_longest_edge
    from dolfinx_eqlb_amd.mesh.refine import closure_by_sweeping
    mesh = sq40()
    for level in range(4):
        marked = level_marks(mesh.ncells, level)
        assert np.array_equal(closure_by_sweeping(mesh, marked), closure_by_doubling(mesh, marked)[0])
        x2, c2, pc, npf = refine_longest_edge(mesh, marked)
        a_old, a_new = _area2(mesh.x, mesh.cell_nodes), _area2(x2, c2)
        assert np.allclose(np.bincount(pc, weights=a_new), a_old, rtol=1e-12, atol=0)
        mesh = create_mesh(x2, c2)
        assert np.diff(mesh.facet_cells_offsets).max() <= 2


def test_marked_ids_are_checked():
    mesh, _ = case("sq3_cell5")
    from dolfinx_eqlb_amd.mesh import refine_longest_edge
    for bad in ([3, mesh.ncells], [-1, 3]):
        with pytest.raises(ValueError, match="marked cell"):
            refine_longest_edge(mesh, bad)
