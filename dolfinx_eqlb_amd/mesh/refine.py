"""Refinement of marked cells by longest-edge closure and bisection - the statement of the rule.

The adaptive demos of the reference call `mesh.refine(mesh, edges)` with the edges of the Dörfler-marked cells
(demo/poisson_adaptive/demo_lshape.py, demo_discont-coeff.py, demo/elasticity_adaptive/demo_cook.py).  The numbering of
that call cannot be pinned here, so this file defines the result; the device path (eqlb_mesh_refine_plan and the
eqlb_refine_* entries of include/eqlb.h) reproduces it bit for bit.

  length   len2[f] = dx*dx + dy*dy, dx = x[hi] - x[lo] from the facet's two nodes, every operation rounded on its own
  order    facet f is longer than g if len2[f] > len2[g], or if they are equal and f < g (global and strict);
           L(c) is the longest facet of cell c in that order, l(c) its local index
  seed     E0 = every facet of every marked cell
  closure  the smallest E that contains E0 in which every cell with a facet in E has L(c) in E
  nodes    one per facet of E, numbered nnodes + rank among E in ascending facet id, at 0.5 * (x[lo] + x[hi])
  cells    a cell without a facet in E is copied.  Otherwise, with l = l(c), a = v[l], b = v[(l+1)%3], c' = v[(l+2)%3],
           m the new node of local facet l, q that of local facet (l+1)%3 and p that of (l+2)%3 where they are in E:
           (a,p,m), (p,b,m) if p exists, else (a,b,m); then (a,m,q), (q,m,c') if q exists, else (a,m,c').
           The children of cell c start at the exclusive prefix sum of 1 + (number of its facets in E).

With every cell marked this is the longest-edge 4-split, not a red refinement.

Between the facets of the two meshes: parent_facets (eqlb_refine_parent_facets), and from it carry_facet_types
(eqlb_refine_facet_types: the type table of the equilibrator on the refined mesh) and its inverse for facet lists,
child_facets (eqlb_refine_child_facets); carry_robin_list states Refinement.carry_robin on top of it, and
carry_springs_list states Refinement.carry_springs.
"""

import numpy as np


def facet_len2(mesh):
    """Squared facet lengths, each operation rounded on its own (no fused multiply-add)."""
    lo, hi = mesh.facet_nodes[:, 0], mesh.facet_nodes[:, 1]
    dx = mesh.x[hi, 0] - mesh.x[lo, 0]
    dy = mesh.x[hi, 1] - mesh.x[lo, 1]
    return dx * dx + dy * dy


def longest_facets(mesh):
    """(l, L): local index and id of the longest facet of every cell in the strict order of the rule."""
    cf = mesh.cell_facets.astype(np.int64)
    len2 = facet_len2(mesh)
    l = np.zeros(mesh.ncells, dtype=np.int64)
    best = cf[:, 0].copy()
    for j in (1, 2):
        f = cf[:, j]
        longer = (len2[f] > len2[best]) | ((len2[f] == len2[best]) & (f < best))
        l[longer] = j
        best[longer] = f[longer]
    return l, best


def _checked(mesh, marked):
    marked = np.asarray(marked, dtype=np.int64).ravel()
    bad = marked[(marked < 0) | (marked >= mesh.ncells)]
    if bad.size:
        raise ValueError(f"refine_longest_edge: marked cell {int(bad.min())} outside [0, {mesh.ncells})")
    return marked


def closure_by_sweeping(mesh, marked, return_passes=False):
    """The closure E [nfacets] bool, by sweeping over the cells until nothing changes."""
    marked = _checked(mesh, marked)
    _, L = longest_facets(mesh)
    E = np.zeros(mesh.nfacets, dtype=bool)
    E[mesh.cell_facets[marked].ravel()] = True
    passes = 0
    while True:
        need = L[E[mesh.cell_facets].any(axis=1)]
        if E[need].all():
            break
        E[need] = True
        passes += 1
    return (E, passes) if return_passes else E


def refine_longest_edge(mesh, marked):
    """(x2 [nnodes2, 3], cell_nodes2 [ncells2, 3] int32, parent_cell [ncells2] int32,
    node_parent_facet [nnodes2 - nnodes] int32) of `mesh` refined at the cells `marked` (duplicates allowed)."""
    E = closure_by_sweeping(mesh, marked)
    nn, nc = mesh.nnodes, mesh.ncells
    l, _ = longest_facets(mesh)
    npf = np.nonzero(E)[0].astype(np.int32)
    new_node = nn + np.cumsum(E) - E                      # id of the node of facet f where E[f]
    lo, hi = mesh.facet_nodes[npf, 0], mesh.facet_nodes[npf, 1]
    x2 = np.concatenate([mesh.x, 0.5 * (mesh.x[lo] + mesh.x[hi])])

    cf = mesh.cell_facets.astype(np.int64)
    Ec = E[cf]
    nch = 1 + Ec.sum(axis=1)
    off = np.cumsum(nch) - nch
    nc2 = int(nch.sum())
    cells2 = np.empty((nc2, 3), dtype=np.int64)
    parent_cell = np.repeat(np.arange(nc, dtype=np.int32), nch)

    rows = np.arange(nc)
    v = mesh.cell_nodes.astype(np.int64)
    cut = Ec.any(axis=1)
    cells2[off[~cut]] = v[~cut]
    l1, l2 = (l + 1) % 3, (l + 2) % 3
    a, b, c = v[rows, l], v[rows, l1], v[rows, l2]
    m, q, p = new_node[cf[rows, l]], new_node[cf[rows, l1]], new_node[cf[rows, l2]]
    has_q, has_p = cut & Ec[rows, l1], cut & Ec[rows, l2]

    def put(mask, pos, n0, n1, n2):
        cells2[pos[mask]] = np.stack([n0[mask], n1[mask], n2[mask]], axis=1)

    put(has_p, off, a, p, m)
    put(has_p, off + 1, p, b, m)
    put(cut & ~has_p, off, a, b, m)
    second = off + 1 + has_p
    put(has_q, second, a, m, q)
    put(has_q, second + 1, q, m, c)
    put(cut & ~has_q, second, a, m, c)
    return x2, cells2.astype(np.int32), parent_cell, npf


def parent_facets(mesh, node_parent_facet, mesh2):
    """parent_facet [nfacets2] int32 of the refined mesh `mesh2` (in its own facet numbering): the old facet if the
    new facet is an unbisected old facet; the bisected old facet if exactly one end is a new node and the other end is
    an end of the facet that node bisects; -1 otherwise (interior new edges)."""
    nn = mesh.nnodes
    npf = np.asarray(node_parent_facet, dtype=np.int64)
    fn2 = mesh2.facet_nodes.astype(np.int64)
    lo, hi = fn2.min(axis=1), fn2.max(axis=1)
    out = np.full(mesh2.nfacets, -1, dtype=np.int32)

    fn = mesh.facet_nodes.astype(np.int64)
    keys = fn.min(axis=1) * nn + fn.max(axis=1)
    order = np.argsort(keys, kind="stable")
    both_old = hi < nn
    k2 = lo[both_old] * nn + hi[both_old]
    pos = np.minimum(np.searchsorted(keys[order], k2), keys.size - 1)
    out[both_old] = np.where(keys[order][pos] == k2, order[pos], -1)

    one_new = (lo < nn) & (hi >= nn)
    g = npf[hi[one_new] - nn]
    on_parent = (fn[g, 0] == lo[one_new]) | (fn[g, 1] == lo[one_new])
    out[one_new] = np.where(on_parent, g, -1)
    return out


def carry_facet_types(facet_type, parent_facet):
    """facet_type2 [nrhs, nfacets2] int8 (or 1-D) of the refined mesh: the type of the parent facet, EQLB_FACET_INTERNAL
    (0) where a facet has none (parent_facet < 0) - the statement of eqlb_refine_facet_types.  Any old value is copied
    as it is."""
    ft = np.asarray(facet_type, dtype=np.int8)
    pf = np.asarray(parent_facet, dtype=np.int64)
    if ft.shape[-1] == 0:
        return np.zeros(ft.shape[:-1] + (pf.size,), dtype=np.int8)
    return np.where(pf < 0, np.int8(0), ft[..., np.maximum(pf, 0)]).astype(np.int8)


def child_facets(mesh, node_parent_facet, mesh2, facets=None):
    """children [n, 2] int32 of the old facets `facets` (None: all of them) in the facet numbering of the refined mesh
    `mesh2` - the inverse of parent_facets, for facet lists.  An old facet with the nodes lo < hi that is not bisected
    has (facet(lo, hi), -1); one bisected by the new node m has (facet(lo, m), facet(m, hi)).  A pair that is no facet
    of mesh2 gives -1 (a mesh2 that is not the refined mesh)."""
    nn, nn2 = mesh.nnodes, mesh2.nnodes
    f = np.arange(mesh.nfacets, dtype=np.int64) if facets is None else np.asarray(facets, dtype=np.int64).ravel()
    bad = f[(f < 0) | (f >= mesh.nfacets)]
    if bad.size:
        raise ValueError(f"child_facets: facet {int(bad[0])} outside [0, {mesh.nfacets})")
    npf = np.asarray(node_parent_facet, dtype=np.int64)
    new_node = np.full(mesh.nfacets, -1, dtype=np.int64)
    new_node[npf] = nn + np.arange(npf.size)
    fn = mesh.facet_nodes.astype(np.int64)
    lo, hi = fn[f].min(axis=1), fn[f].max(axis=1)
    m = new_node[f]

    fn2 = mesh2.facet_nodes.astype(np.int64)
    keys = fn2.min(axis=1) * nn2 + fn2.max(axis=1)
    order = np.argsort(keys, kind="stable")

    def find(a, b):
        k = np.minimum(a, b) * nn2 + np.maximum(a, b)
        pos = np.minimum(np.searchsorted(keys[order], k), keys.size - 1)
        return np.where(keys[order][pos] == k, order[pos], -1)

    cut = m >= 0
    first = np.where(cut, find(lo, np.where(cut, m, hi)), find(lo, hi))
    second = np.where(cut, find(np.where(cut, m, lo), hi), -1)
    return np.stack([first, second], axis=1).astype(np.int32)


def _carry_facet_list(mesh, node_parent_facet, mesh2, f, values):
    """The rule of a facet list with one row of values per facet across a refinement: the children of every listed facet
    through child_facets, in the order of the list, first child first, the -1 of an unbisected facet left out; the
    parent's row of values [nlist, ...] is copied to both."""
    ch = child_facets(mesh, node_parent_facet, mesh2, f)
    keep = ch >= 0
    return ch[keep].astype(np.int32), np.repeat(values[:, None], 2, axis=1)[keep]


def carry_robin_list(mesh, node_parent_facet, mesh2, facets, facet_alpha):
    """(facets2 int32, facet_alpha2) of a Robin list (PoissonOperator.set_robin) on the refined mesh `mesh2` - the
    statement of Refinement.carry_robin: the children of every listed facet through child_facets, in the order of the
    list, first child first, the -1 of an unbisected facet left out; a child takes its parent's alpha."""
    f = np.asarray(facets, dtype=np.int64).ravel()
    a = np.asarray(facet_alpha, dtype=np.float64).ravel()
    if a.size != f.size:
        raise ValueError("carry_robin_list: facet_alpha [nlist] expected")
    return _carry_facet_list(mesh, node_parent_facet, mesh2, f, a)


def carry_springs_list(mesh, node_parent_facet, mesh2, facets, facet_k):
    """(facets2 int32, facet_k2 [n2, 3]) of a spring list (ElasticityOperator.set_springs) on the refined mesh `mesh2` -
    the statement of Refinement.carry_springs: the rule of carry_robin_list, and a child takes its parent's tensor K as
    it is: K is stated in global axes, and a child of a straight facet has its parent's normal, so nothing is
    rotated."""
    f = np.asarray(facets, dtype=np.int64).ravel()
    K = np.asarray(facet_k, dtype=np.float64)
    if K.size != 3 * f.size:
        raise ValueError("carry_springs_list: facet_k [nlist][3] expected")
    return _carry_facet_list(mesh, node_parent_facet, mesh2, f, K.reshape(f.size, 3))
