"""Shared by tests/test_primal_meshes_host.py and tests/test_gpu_primal_meshes.py: the meshes, hierarchies, boundary
layouts, data and solve cases that carry the checks of the P_p solvers (Poisson, elasticity, the multilevel
preconditioner) beyond the perturbed unit square.  No test lives here.  Every mesh comes from a generator of the tree;
its counts are asserted when it is built, so a change of a generator cannot quietly empty a case.

What each mesh is there for:

  disk100      a vertex of 100 cells: the slot loop of the sum pass far beyond the 8 slots of a crossed square
  hole         a second boundary loop (Dirichlet all around, or on the inner loop only)
  two_parts    two components, each with its own Dirichlet boundary
  lshape       a re-entrant corner (the base of the graded hierarchy)
  bowtie       two quadrants that meet in one pinched vertex
  delaunay     an unstructured Delaunay mesh of an ellipse: valences 3 ... 10, no structure in the numbering
  tiny_far     base9 scaled by 1e-6 and moved to 250: det ~ 1e-14, 1 / det ~ 1e14, coordinates that cancel
  huge         base9 scaled by 1e5: det ~ 1e8
  aspect1000   base9 stretched by 1000 in x: K K^T with entries six orders of magnitude apart
  wg128/256/512  cell counts that are whole workgroups of the cell kernels (128 per workgroup for elasticity, 256 for
               Poisson): no partial last workgroup
  triangle, right1  one cell, two cells: spaces with no or hardly any free row
  sq91         33 124 cells: more rows than one pass of the streaming kernels (512 blocks of 256 = 131 072) at
               Poisson p = 3 (149 605) and elasticity p = 2 (133 226)

base9 is create_unit_square(9, shuffle_seed=3, perturb=0.15), the base mesh of the other primal tests."""

import zlib

import numpy as np

import elasticity_cases as ec
import multilevel_cases as mc
import primal_cases as pc
import refine_cases
import topology_meshes

# name -> (cells, nodes, largest number of cells at a vertex; None: not pinned)
COUNTS = {"disk100": (300, 201, 100), "hole": (192, 120, 8), "two_parts": (192, 120, 8), "lshape": (192, 113, 8),
          "bowtie": (128, 81, 8), "delaunay": (658, 360, 10), "tiny_far": (324, 181, 8), "huge": (324, 181, 8),
          "aspect1000": (324, 181, 8), "wg128": (128, 77, 8), "wg256": (256, 145, 8), "wg512": (512, 281, 8),
          "triangle": (1, 3, None), "right1": (2, 4, None), "sq91": (33124, 16745, 8)}
SINGLE = [n for n in COUNTS if n not in ("sq91", "triangle", "right1")]      # the meshes of the bit-for-bit table
ROWS_PER_PASS = 512 * 256

_MESHES, _LEVELS = {}, {}


def valence(mesh):
    return int(np.diff(mesh.node_cells_offsets).max())


def _base9():
    from dolfinx_eqlb_amd.mesh import create_unit_square
    return create_unit_square(9, shuffle_seed=3, perturb=0.15)


def _moved(change):
    from dolfinx_eqlb_amd.mesh import create_mesh
    base = _base9()
    return create_mesh(change(base.x[:, :2].copy()), base.cell_nodes)


def _stretch(x):
    x[:, 0] *= 1000.0
    return x


def mesh_of(name):
    if name in _MESHES:
        return _MESHES[name]
    from dolfinx_eqlb_amd.mesh import create_disk, create_rectangle, create_unit_square
    if name == "disk100":
        mesh = create_disk(100, 2, shuffle_seed=3)
    elif name in ("hole", "two_parts", "lshape", "bowtie"):
        mesh = topology_meshes.mesh_of(name)
    elif name == "delaunay":
        from test_gpu_unstructured import delaunay_mesh
        mesh = delaunay_mesh(300, seed=2)
    elif name == "tiny_far":
        mesh = _moved(lambda x: x * 1e-6 + 250.0)
    elif name == "huge":
        mesh = _moved(lambda x: x * 1e5)
    elif name == "aspect1000":
        mesh = _moved(_stretch)
    elif name in ("wg128", "wg256", "wg512"):
        nx, ny = {"wg128": (4, 8), "wg256": (8, 8), "wg512": (8, 16)}[name]
        mesh = create_rectangle(nx, ny, shuffle_seed=3, perturb=0.15)
    elif name in ("triangle", "right1"):
        mesh = refine_cases.case(name)[0]
    elif name == "sq91":
        mesh = create_unit_square(91, shuffle_seed=3, perturb=0.15)
    else:
        raise KeyError(name)
    ncells, nnodes, val = COUNTS[name]
    assert mesh.ncells == ncells, (name, mesh.ncells)
    assert nnodes is None or mesh.nnodes == nnodes, (name, mesh.nnodes)
    assert val is None or valence(mesh) == val, (name, valence(mesh))
    if name in ("wg128", "wg256", "wg512"):
        assert mesh.ncells % 128 == 0
    if name in ("tiny_far", "huge", "aspect1000"):
        assert np.array_equal(mesh.cell_nodes, _base9().cell_nodes)
    _MESHES[name] = mesh
    return mesh


# ---- hierarchies -----------------------------------------------------------------------------------------------------------
def _corner_cells(mesh):
    """the cells of the vertex nearest (0.5, 0.5): the re-entrant corner of `lshape`"""
    v = int(np.argmin(np.sum((mesh.x[:, :2] - 0.5) ** 2, axis=1)))
    return np.sort(mesh.node_cells[mesh.node_cells_offsets[v]:mesh.node_cells_offsets[v + 1]]).astype(np.int32)


def _all(mesh):
    return mc.all_cells(mesh.ncells)


def _fixed(marked):
    return lambda mesh: np.asarray(marked, dtype=np.int32)


# name -> (cells per level, the sorted numbers of children a parent has, per link)
LEVEL_COUNTS = {
    "disk70": ([210, 226, 904], [[1, 2, 3, 4], [4]]),
    "hole": ([192, 429, 1716], [[1, 2, 3, 4], [4]]),
    "lshape_graded": ([192, 228, 264, 300, 316, 358, 421, 469, 487],
                      [[1, 2, 3, 4]] * 3 + [[1, 2, 4]] + [[1, 2, 3, 4]] * 4),
    "sq6_two": ([144, 172], [[1, 2, 3, 4]]),
}


def levels_of(name):
    """(base mesh, marks): marks[l](mesh of level l) are the cells refined there (int32)"""
    from dolfinx_eqlb_amd.mesh import create_unit_square
    if name == "disk70":
        base, marked = refine_cases.case("disk")
        return base, [_fixed(marked), _all]
    if name == "hole":
        base, marked = refine_cases.case("hole")
        assert np.array_equal(marked, np.arange(0, base.ncells, 7))
        return base, [_fixed(marked), _all]
    if name == "lshape_graded":
        return mesh_of("lshape"), [_corner_cells] * 8
    if name == "sq6_two":
        base = create_unit_square(6, shuffle_seed=3, perturb=0.15)
        return base, [_fixed(refine_cases.level_marks(base.ncells, 1))]
    raise KeyError(name)


def check_levels(name, meshes, links):
    """the counts of LEVEL_COUNTS on meshes [L + 1] and links [L] = (parent_cell, node_parent_facet)"""
    cells, children = LEVEL_COUNTS[name]
    assert len(meshes) == len(cells) and len(links) == len(children)
    for m, n in zip(meshes, cells):
        assert n is None or m.ncells == n, (name, [q.ncells for q in meshes])
    for l, (link, kids) in enumerate(zip(links, children)):
        got = sorted(set(np.bincount(np.asarray(link[0]), minlength=meshes[l].ncells)))
        assert got == kids, (name, l, got)
    if name == "disk70":
        assert all(valence(m) >= 70 for m in meshes)
    if name == "lshape_graded":
        assert sum(m.ncells < 256 for m in meshes) == 2


def levels_host(name):
    """(meshes, links) refined on the host by mesh.refine.refine_longest_edge, checked against LEVEL_COUNTS"""
    if name not in _LEVELS:
        base, marks = levels_of(name)
        meshes, links = [base], []
        for mk in marks:
            m2, pcell, npf = mc.refine_host(meshes[-1], mk(meshes[-1]))
            meshes.append(m2)
            links.append((pcell, npf))
        check_levels(name, meshes, links)
        _LEVELS[name] = (meshes, links)
    return _LEVELS[name]


# ---- boundary layouts ------------------------------------------------------------------------------------------------------
def dirichlet_facets(mesh, layout):
    """"all": every boundary facet.  "inner": the inner loop of `hole` (of a refinement of it: the boundary facets away
    from the sides of the unit square).  "part": the boundary facets whose midpoint lies left of the middle of the mesh;
    the rest of the boundary is free (natural)."""
    bf = mesh.boundary_facets()
    if layout == "all":
        return bf
    if layout == "inner":
        return topology_meshes.inner_loop_facets(mesh)
    assert layout == "part"
    mp = mesh.facet_midpoints()[bf]
    return bf[mp[:, 0] < 0.5 * (mesh.x[:, 0].min() + mesh.x[:, 0].max())]


def quadrant_sides(mesh):
    """four lists of boundary facets by the quadrant of the midpoint's angle round the middle of the bounding box: what
    the four sides of the unit square are to galerkin.side_facets, on any mesh"""
    bf = mesh.boundary_facets()
    mid = 0.5 * (mesh.x[:, :2].min(axis=0) + mesh.x[:, :2].max(axis=0))
    d = mesh.facet_midpoints()[bf][:, :2] - mid
    q = (np.floor(np.arctan2(d[:, 1], d[:, 0]) / (0.5 * np.pi)).astype(np.int64) + 2) % 4
    return [bf[q == s] for s in range(4)]


def elasticity_lists(mesh, layout):
    """the two facet lists of PrimalElasticity.set_dirichlet: "all", or "mixed": the flags MIXED of
    tests/test_gpu_primal_elasticity.py on quadrant_sides (row 0 free on side 0, row 1 on side 1, both on side 2)"""
    ft = np.zeros((2, mesh.nfacets), dtype=np.int8)
    ft[:, mesh.boundary_facets()] = 1
    if layout == "mixed":
        from test_gpu_primal_elasticity import MIXED
        sides = quadrant_sides(mesh)
        assert all(s.size > 0 for s in sides)
        for s, flags in enumerate(MIXED):
            for r in range(2):
                if flags[r]:
                    ft[r, sides[s]] = 2
    else:
        assert layout == "all"
    return ec.dirichlet_lists(ft)


# ---- operators and data --------------------------------------------------------------------------------------------------
def seed_of(*key):
    return zlib.crc32("-".join(str(k) for k in key).encode())


def statement(problem, mesh, p, layout="all", coeff=None):
    """(the numpy statement with its mask, the coefficient [ncells], the arguments of set_dirichlet)"""
    from dolfinx_eqlb_amd.lsolver import primal
    if problem == "poisson":
        coeff = pc.kappa_of(mesh.ncells) if coeff is None else coeff
        args = (dirichlet_facets(mesh, layout),)
        op = primal.PoissonOperator(mesh, p, coeff)
    else:
        coeff = ec.pi1_of(mesh.ncells) if coeff is None else coeff
        args = tuple(elasticity_lists(mesh, layout))
        op = primal.ElasticityOperator(mesh, p, cell_pi1=coeff)
    op.set_dirichlet(*args)
    return op, coeff, args


def vectors(problem, mesh, p, n, key):
    """u, e [n] and the DG_d data f of the bit-for-bit checks, d = min(p, 3)"""
    rng = np.random.default_rng(seed_of("bits", problem, key, p))
    d = min(p, 3)
    nf = mesh.ncells * (d + 1) * (d + 2) // 2
    f = rng.standard_normal(nf) if problem == "poisson" else rng.standard_normal((2, nf))
    return dict(d=d, f=f, e=rng.standard_normal(n), u=rng.standard_normal(n))


def solve_data(op, problem, key, p, inhomogeneous=False):
    """(b, u0, start): a random right-hand side on the free rows; u0 = 0, or random Dirichlet values with any start on
    the free rows"""
    n = op.fixed.size
    rng = np.random.default_rng(seed_of("solve", problem, key, p))
    b = np.where(op.fixed, 0.0, rng.standard_normal(n))
    if not inhomogeneous:
        return b, np.zeros(n), np.zeros(n)
    u0 = np.where(op.fixed, rng.standard_normal(n), 0.0)
    return b, u0, np.where(op.fixed, u0, rng.standard_normal(n))


def assembled(problem, mesh, p, coeff):
    if problem == "poisson":
        return pc.assemble(mesh, p, coeff)[0]
    return ec.assemble(mesh, p, 1.0, coeff)[0]


def allowance(iterations):
    """the allowance of the other primal tests for the rounding of the inner products"""
    return max(2, iterations // 20)


# ---- the solve cases -----------------------------------------------------------------------------------------------------
# (problem, mesh, p, layout, iterations of the statement, in_allowance).  The count is that of the statement's own PCG
# (op.pcg, rtol 1e-10) on the data of solve_data; a device solve gets maxit = 2 * count: a cap against a silent crawl,
# not a tolerance - operator and diagonal are pinned bit for bit, the device differs in the order of the inner-product
# sums alone.  in_allowance: the statement run once more with every inner product summed over the reversed vectors
# stays within allowance() of the count - only there is the device's count asserted against it, elsewhere it is printed.
# (The reversed runs moved a count by 7 of 2236 at the most, so every case below is asserted.)  Both columns are what
# statement_counts() below prints on the CPU (two minutes); tests/test_primal_meshes_host.py re-runs the short ones.
SINGLE_SOLVES = [
    ("poisson", "disk100", 1, "all", 108, True),
    ("poisson", "disk100", 2, "all", 454, True),
    ("poisson", "disk100", 4, "all", 1580, True),
    ("poisson", "bowtie", 4, "all", 313, True),
    ("poisson", "two_parts", 4, "all", 367, True),
    ("poisson", "hole", 4, "all", 309, True),
    ("poisson", "delaunay", 2, "all", 337, True),
    ("poisson", "delaunay", 3, "all", 652, True),
    ("poisson", "tiny_far", 2, "all", 169, True),
    ("poisson", "tiny_far", 4, "all", 562, True),
    ("poisson", "huge", 2, "all", 169, True),
    ("poisson", "huge", 4, "all", 564, True),
    ("poisson", "aspect1000", 2, "all", 533, True),
    ("poisson", "aspect1000", 4, "all", 2236, True),
    ("elasticity", "disk100", 2, "all", 1233, True),
    ("elasticity", "bowtie", 2, "all", 192, True),
    ("elasticity", "tiny_far", 2, "all", 373, True),
    ("elasticity", "aspect1000", 2, "all", 395, True),
    ("poisson", "disk100", 2, "part", 545, True),
    ("elasticity", "delaunay", 2, "mixed", 1133, True),
]
# (problem, hierarchy, p, levels used, iterations of the statement Hierarchy.pcg, in_allowance)
HIERARCHY_SOLVES = [
    ("poisson", "disk70", 1, 3, 254, True),
    ("poisson", "disk70", 2, 3, 402, True),
    ("poisson", "hole", 1, 3, 55, True),
    ("poisson", "hole", 3, 2, 188, True),
    ("poisson", "lshape_graded", 1, 9, 66, True),
    ("poisson", "lshape_graded", 2, 9, 132, True),
    ("poisson", "lshape_graded", 3, 9, 258, True),
    ("elasticity", "lshape_graded", 2, 9, 297, True),
    ("elasticity", "sq6_two", 3, 2, 441, True),
    ("elasticity", "sq6_two", 4, 2, 752, True),
]
# the smallest meshes: (mesh, p, free rows, iterations of the statement; None where no row is free)
SMALLEST = [("triangle", 1, 0, None), ("triangle", 2, 0, None), ("triangle", 3, 1, 1), ("triangle", 4, 3, 3),
            ("right1", 1, 0, None), ("right1", 2, 1, 1), ("right1", 3, 4, 4), ("right1", 4, 9, 9)]


def case_id(case):
    return "-".join(str(c) for c in case[:4])


def host_hierarchy(problem, name, p, nlevels):
    """(Hierarchy of the statements with Dirichlet conditions all around, meshes, coefficients) on the first `nlevels`
    levels of levels_host(name)"""
    meshes, links = levels_host(name)
    meshes, links = meshes[:nlevels], links[:nlevels - 1]
    coeff = mc.coefficients(meshes, links, pc.kappa_of if problem == "poisson" else ec.pi1_of)
    ops = [statement(problem, m, p, "all", k)[0] for m, k in zip(meshes, coeff)]
    return mc.Hierarchy(ops, links), meshes, coeff


class _ReversedSums:
    """numpy with sum(x) taken over the reversed vector: another order of the inner products of a PCG statement"""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def sum(x, *args, **kwargs):
        return np.sum(np.asarray(x)[::-1].copy(), *args, **kwargs)


def _count(pcg, b, start, reverse, modules):
    saved = [m.np for m in modules]
    try:
        if reverse:
            for m in modules:
                m.np = _ReversedSums()
        return pcg(b, start, rtol=1e-10, maxit=20000)[1]["iterations"]
    finally:
        for m, s in zip(modules, saved):
            m.np = s


def statement_counts(which=("single", "hierarchy")):
    """prints the two columns of SINGLE_SOLVES and HIERARCHY_SOLVES (CPU, a few minutes)"""
    from dolfinx_eqlb_amd.lsolver import multilevel, primal
    if "single" in which:
        for case in SINGLE_SOLVES:
            problem, name, p, layout = case[:4]
            op = statement(problem, mesh_of(name), p, layout)[0]
            b, _, start = solve_data(op, problem, name, p, layout != "all")
            n, r = (_count(op.pcg, b, start, rev, [primal]) for rev in (False, True))
            print(f'    ("{problem}", "{name}", {p}, "{layout}", {n}, {abs(n - r) <= allowance(r)}),    # reversed {r}',
                  flush=True)
    if "hierarchy" in which:
        for case in HIERARCHY_SOLVES:
            problem, name, p, nlevels = case[:4]
            H = host_hierarchy(problem, name, p, nlevels)[0]
            b, _, start = solve_data(H.ops[-1], problem, name, p)
            n, r = (_count(H.pcg, b, start, rev, [primal, multilevel]) for rev in (False, True))
            print(f'    ("{problem}", "{name}", {p}, {nlevels}, {n}, {abs(n - r) <= allowance(r)}),    # reversed {r}',
                  flush=True)
