"""Meshes whose boundary is more than one simple loop, and the boundary-condition layouts the topology tests put on
them (tests/test_gpu_topology.py, tests/test_gpu_partition.py).

All of them are sub-meshes of create_unit_square(8, shuffle_seed=5, perturb=0.2): cells are kept or dropped by the
centroid they have in the UNPERTURBED 8 x 8 crossed square (same cell order), so the selection does not depend on
the perturbation.  The counts the cases rest on are asserted here: a change of the generator cannot quietly empty a
case.

  hole       a second boundary loop of 16 facets round the middle, 4 boundary vertices of 6 cells at its corners
  two_holes  three boundary loops
  lshape     one re-entrant corner of 6 cells
  two_parts  two components (a strip of the square dropped), 8 two-cell corners
  bowtie     two quadrants that meet in the centre vertex only: one vertex with two open fans (4 cells, 6 facets)
"""

import numpy as np

N = 8
TILE_SMALL = 31     # option "tile_cells" of the second tiled run: tiles straddle holes, corners and the gap

DROP = {
    "hole": lambda x, y: (np.abs(x - .5) < .25) & (np.abs(y - .5) < .25),
    "two_holes": lambda x, y: ((np.abs(x - .25) < .125) & (np.abs(y - .25) < .125))
    | ((np.abs(x - .75) < .125) & (np.abs(y - .625) < .25)),
    "lshape": lambda x, y: (x > .5) & (y > .5),
    "two_parts": lambda x, y: np.abs(x - .5) <= .125,
    "bowtie": lambda x, y: ((x > .5) & (y > .5)) | ((x < .5) & (y < .5)),
}
# (cells, nodes, boundary loops, components)
COUNTS = {"hole": (192, 120, 2, 1), "two_holes": (208, 129, 3, 1), "lshape": (192, 113, 1, 1),
          "two_parts": (192, 120, 2, 2), "bowtie": (128, 81, None, 1)}
NAMES = ["hole", "two_holes", "lshape", "two_parts"]      # the meshes every node of which can be equilibrated
LAYOUTS = ["dirichlet", "flux_bottom", "flux_middle"]


def submesh(base, keep):
    """Mesh of the kept cells of `base` (bool [ncells]); the used nodes are renumbered in ascending order, the cells
    keep their order and their local vertex order."""
    from dolfinx_eqlb_amd.mesh import create_mesh
    cn = base.cell_nodes[np.asarray(keep, dtype=bool)]
    used = np.unique(cn)
    remap = -np.ones(base.nnodes, dtype=np.int32)
    remap[used] = np.arange(used.size, dtype=np.int32)
    return create_mesh(base.x[used, :2], remap[cn])


def node_counts(mesh):
    """(cells, facets, one-cell facets) per node."""
    n = np.diff(mesh.node_cells_offsets)
    nf = np.diff(mesh.node_facets_offsets)
    b = np.zeros(mesh.nnodes, dtype=np.int64)
    np.add.at(b, mesh.facet_nodes[mesh.boundary_facets()].ravel(), 1)
    return n, nf, b


def boundary_loops(mesh):
    """Number of closed loops of the boundary facets (every boundary vertex has two of them)."""
    bf = mesh.boundary_facets()
    parent = {int(v): int(v) for v in np.unique(mesh.facet_nodes[bf])}

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    for a, b in mesh.facet_nodes[bf]:
        parent[find(int(a))] = find(int(b))
    return len({find(v) for v in parent})


def components(mesh):
    parent = np.arange(mesh.nnodes)

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    for a, b, c in mesh.cell_nodes:
        parent[find(a)] = find(b)
        parent[find(c)] = find(b)
    return len({find(v) for v in range(mesh.nnodes)})


_MESHES = {}


def mesh_of(name):
    if name in _MESHES:
        return _MESHES[name]
    from dolfinx_eqlb_amd.mesh import create_unit_square
    base = create_unit_square(N, shuffle_seed=5, perturb=0.2)
    plain = create_unit_square(N)
    assert np.array_equal(np.sort(plain.cell_nodes, axis=1), np.sort(base.cell_nodes, axis=1))
    cen = plain.x[plain.cell_nodes, :2].mean(axis=1)
    mesh = submesh(base, ~DROP[name](cen[:, 0], cen[:, 1]))
    ncells, nnodes, nloops, ncomp = COUNTS[name]
    assert (mesh.ncells, mesh.nnodes) == (ncells, nnodes), (name, mesh.ncells, mesh.nnodes)
    assert components(mesh) == ncomp
    n, nf, b = node_counts(mesh)
    if name == "bowtie":
        pinched = np.nonzero(nf - n >= 2)[0]
        assert pinched.size == 1 and (n[pinched[0]], nf[pinched[0]], b[pinched[0]]) == (4, 6, 4)
    else:
        assert np.all(((nf == n) & (b == 0)) | ((nf == n + 1) & (b == 2))) and n.min() >= 2
        assert boundary_loops(mesh) == nloops
        assert mesh.ncells < 448      # below one default tile of every launch
    if name == "hole":
        inner = inner_loop_facets(mesh)
        assert inner.size == 16
        assert np.count_nonzero((b == 2) & (n == 6)) == 4
    if name == "lshape":
        assert np.count_nonzero((b == 2) & (n == 6)) == 1
    if name == "two_parts":
        assert np.count_nonzero((b == 2) & (n == 2)) == 8
    _MESHES[name] = mesh
    return mesh


def inner_loop_facets(mesh):
    """Boundary facets away from the sides of the unit square."""
    bf = mesh.boundary_facets()
    mp = mesh.facet_midpoints()[bf]
    return bf[(np.abs(mp[:, 0] - .5) < .45) & (np.abs(mp[:, 1] - .5) < .45)]


def pinched_node(mesh):
    n, nf, _ = node_counts(mesh)
    return int(np.nonzero(nf - n >= 2)[0][0])


def _bottom(p):
    outer = (np.abs(p[:, 0] - .5) > .45) | (np.abs(p[:, 1] - .5) > .45)
    return outer & (p[:, 1] < p[:, 1].min() + 0.3)


def _middle(p):
    return (np.abs(p[:, 0] - .5) < .3) & (np.abs(p[:, 1] - .5) < .3)


NEUMANN = {"dirichlet": None, "flux_bottom": _bottom, "flux_middle": _middle}
# flux-BC facets of the third layout (on `hole` the whole inner loop: every boundary patch round the hole is pure
# flux-BC)
MIDDLE_FACETS = {"hole": 16, "two_holes": 6, "lshape": 4, "two_parts": 8}


def facet_table(mesh, layout):
    """[1, nfacets] facet types of a layout: all primal-Dirichlet | flux BCs on the outer facets with y < ymin + 0.3 |
    flux BCs on every boundary facet with |x - .5| < .3 and |y - .5| < .3."""
    from synthetic import facet_types
    return facet_types(mesh, NEUMANN[layout])


_CASES = {}


def case(name, layout, k):
    """(mesh, ft [1, nfacets], G [1, .], f [1, .]) with compatible data; built once."""
    key = (name, layout, k)
    if key not in _CASES:
        from synthetic import make_compatible_data
        mesh = mesh_of(name)
        ft = facet_table(mesh, layout)
        if layout == "flux_middle":
            assert np.count_nonzero(ft[0] == 2) == MIDDLE_FACETS[name], (name, np.count_nonzero(ft[0] == 2))
        if layout == "flux_bottom":
            assert np.count_nonzero(ft[0] == 2) > 0
        G, f = make_compatible_data(mesh, k, ft, seed=31)
        _CASES[key] = (mesh, ft, G[None], f[None])
    return _CASES[key]
