"""Transfer of P_p solutions and DG_d data across one refinement level - the statement of the rule.

The adaptive demos of the reference interpolate between the nested meshes of `mesh.refine` (DOLFINx' interpolation of a
Function of the old mesh into the space of the new one).  This file defines the result in numpy; the device path
(eqlb_mesh_lagrange_dofmap, eqlb_refine_prolong_lagrange, eqlb_refine_prolong_dg of include/eqlb.h) reproduces it.

  dofmap    lagrange_dofmap: vertex DOFs are the node ids; facet f carries p-1 DOFs nnodes + f*(p-1) + j ordered from
            its lower to its higher node id; cell c carries ni = (p-1)(p-2)/2 DOFs nnodes + nfacets*(p-1) + c*ni + j
            (local order: elmtlib/lagrange.py)
  lattice   the half-spacing lattice of the reference triangle for degree q: the points (i, j) / (2q), i, j >= 0,
            i + j <= 2q, in the ROW ORDER j ascending, i ascending within j: row(i, j) = j*(2q+1) - j*(j-1)/2 + i
  table     prolong_table(q)[row][k] = value of the equispaced P_q basis function k at that lattice point, computed
            as an exact Fraction and rounded once to double
  position  a child of one bisection level has vertices that are parent vertices or midpoints of parent edges.  With
            the parent vertices at H = (0,0), (2,0), (0,2) (half units), child vertex k sits at h_k = H[j] if it is the
            parent's vertex j, and at (H[ja] + H[jb]) / 2 if it is the new node of the facet with the ends v[ja], v[jb]
            - found by matching node ids, never coordinates.  Local DOF n of the child, at (a_n, b_n) / q of its own
            reference cell, is the lattice point q*h_0 + a_n*(h_1 - h_0) + b_n*(h_2 - h_0) of the parent
  value     sum_i T[row][i] * v_P[i]: every product rounded on its own, added in ascending i
  owner     prolong_lagrange writes each global DOF once: a vertex DOF from the first cell of the node -> cell table of
            the refined mesh, a facet DOF from the first cell of its facet -> cell table, an interior DOF from its cell

DG_0 is the constant: every child takes the value of its parent.

The flux-BC DOF table of the equilibrator crosses the refinement by prolong_flux_bc (eqlb_refine_prolong_flux_bc); its
rule stands in front of it below.
"""

from fractions import Fraction
from functools import lru_cache

import numpy as np

from ..elmtlib.lagrange import Lagrange, lagrange_nodes

_H = np.array([[0, 0], [2, 0], [0, 2]], dtype=np.int64)


def nd_of(d):
    return (d + 1) * (d + 2) // 2


def lagrange_dofmap(mesh, p):
    """(cell_dofs [ncells, nd_p] int32, ndofs) of the conforming P_p space, 1 <= p <= 4."""
    if p < 1 or p > 4:
        raise ValueError(f"lagrange_dofmap: p = {p} outside 1 ... 4")
    nn, nf, nc = mesh.nnodes, mesh.nfacets, mesh.ncells
    ne, ni = p - 1, (p - 1) * (p - 2) // 2
    cd = np.empty((nc, nd_of(p)), dtype=np.int64)
    cd[:, :3] = mesh.cell_nodes
    col = 3
    for f in range(3):
        base = nn + mesh.cell_facets[:, f].astype(np.int64) * ne
        rev = mesh.facet_perm[:, f] == 1
        for j in range(ne):
            cd[:, col] = base + np.where(rev, ne - 1 - j, j)
            col += 1
    for j in range(ni):
        cd[:, col] = nn + nf * ne + np.arange(nc, dtype=np.int64) * ni + j
        col += 1
    return cd.astype(np.int32), nn + nf * ne + nc * ni


def lattice_row(q, i, j):
    """Row of the lattice point (i, j) / (2q) (integers or integer arrays)."""
    return j * (2 * q + 1) - j * (j - 1) // 2 + i


@lru_cache(maxsize=None)
def prolong_table_exact(q):
    """[(2q+1)(2q+2)/2][nd_q] Fractions: P_q basis function k at lattice row r."""
    if q < 1 or q > 4:
        raise ValueError(f"prolong_table: q = {q} outside 1 ... 4")
    basis = Lagrange(q).basis
    rows = []
    for j in range(2 * q + 1):
        for i in range(2 * q + 1 - j):
            x, y = Fraction(i, 2 * q), Fraction(j, 2 * q)
            rows.append(tuple(sum((c * x ** a * y ** b for (a, b), c in phi.items()), Fraction(0)) for phi in basis))
    return tuple(rows)


def prolong_table(q):
    """The table as doubles, each entry rounded once."""
    return np.array([[float(v) for v in row] for row in prolong_table_exact(q)])


def dof_numerators(q):
    """(a_n, b_n) [nd_q, 2]: local DOF n of P_q sits at (a_n, b_n) / q (q >= 1)."""
    return np.array([[int(x * q), int(y * q)] for x, y in lagrange_nodes(q)], dtype=np.int64)


def child_vertex_positions(mesh, mesh2, parent_cell, node_parent_facet):
    """h [ncells2, 3, 2] int: position of every child vertex in its parent, in half units."""
    nn = mesh.nnodes
    pc = np.asarray(parent_cell, dtype=np.int64)
    npf = np.asarray(node_parent_facet, dtype=np.int64)
    v = mesh.cell_nodes[pc].astype(np.int64)
    w = mesh2.cell_nodes.astype(np.int64)
    fn = mesh.facet_nodes.astype(np.int64)
    h = np.zeros((w.shape[0], 3, 2), dtype=np.int64)
    for k in range(3):
        n = w[:, k]
        old = n < nn
        f = npf[np.where(old, 0, n - nn)] if npf.size else np.zeros_like(n)
        for end in (0, 1):
            e = np.where(old, n, fn[f, end])
            match = v == e[:, None]
            if not np.all(match.sum(axis=1) == 1):
                raise ValueError("prolong: a child vertex is neither a vertex nor an edge midpoint of its parent")
            h[:, k] += _H[np.argmax(match, axis=1)]
    return h // 2


def lattice_rows(q, h):
    """r [ncells2, nd_q]: lattice row of every local DOF of every child."""
    ab = dof_numerators(q)
    pos = q * h[:, None, 0, :] + ab[None, :, 0:1] * (h[:, 1] - h[:, 0])[:, None, :] \
        + ab[None, :, 1:2] * (h[:, 2] - h[:, 0])[:, None, :]
    return lattice_row(q, pos[..., 0], pos[..., 1])


def _contract(T, rows, vP):
    """(val, A) [..., ncells2, nd]: sum_i T[rows][i] vP[..., i] in ascending i and sum_i |T| |vP|; vP [..., ncells2, nd]."""
    Tr = T[rows]                                   # [ncells2, nd, nd]
    val = Tr[..., 0] * vP[..., None, 0]
    A = np.abs(Tr[..., 0]) * np.abs(vP[..., None, 0])
    for i in range(1, T.shape[1]):
        val = val + Tr[..., i] * vP[..., None, i]
        A = A + np.abs(Tr[..., i]) * np.abs(vP[..., None, i])
    return val, A


def prolong_dg(mesh, mesh2, parent_cell, node_parent_facet, d, values, bs=1, return_abs=False):
    """values [nrhs, ncells*nd_d*bs] of the old mesh -> [nrhs, ncells2*nd_d*bs] of the refined one (the layout of
    flux_dg with bs = 2, rhs_dg with bs = 1, cell_coeff with d = 0).  return_abs: also A = sum_i |T[r][i]| |v_P[i]|."""
    if d < 0 or d > 3:
        raise ValueError(f"prolong_dg: degree = {d} outside 0 ... 3")
    nd = nd_of(d)
    pc = np.asarray(parent_cell, dtype=np.int64)
    vals = np.asarray(values, dtype=np.float64)
    one = vals.ndim == 1
    v = vals.reshape(-1, mesh.ncells, nd, bs)
    vP = np.moveaxis(v[:, pc], 3, 1)               # [nrhs, bs, ncells2, nd]
    if d == 0:
        out, A = vP.copy(), np.abs(vP)
    else:
        rows = lattice_rows(d, child_vertex_positions(mesh, mesh2, pc, node_parent_facet))
        out, A = _contract(prolong_table(d), rows, vP)
    out, A = [np.ascontiguousarray(np.moveaxis(a, 1, 3)).reshape(v.shape[0], -1) for a in (out, A)]
    if one:
        out, A = out[0], A[0]
    return (out, A) if return_abs else out


def dof_owners(mesh2, p):
    """mask [ncells2, nd_p] bool: the cell is the owner of its local DOF."""
    nc2 = mesh2.ncells
    cells = np.arange(nc2)
    mask = np.ones((nc2, nd_of(p)), dtype=bool)
    for n in range(3):
        mask[:, n] = mesh2.node_cells[mesh2.node_cells_offsets[mesh2.cell_nodes[:, n]]] == cells
    for f in range(3):
        own = mesh2.facet_cells[mesh2.facet_cells_offsets[mesh2.cell_facets[:, f]]] == cells
        mask[:, 3 + f * (p - 1):3 + (f + 1) * (p - 1)] = own[:, None]
    return mask


def prolong_lagrange(mesh, mesh2, parent_cell, node_parent_facet, p, u, cell_dofs=None, cell_dofs2=None, bs=1,
                     ndofs2=None, out=None, return_abs=False):
    """u [nrhs, ndofs*bs] (read as u[r][dof*bs + b]) of the P_p space on the old mesh -> [nrhs, ndofs2*bs] on the
    refined one.  cell_dofs / cell_dofs2: the caller's dofmaps (None: lagrange_dofmap); ndofs2: size of the new space
    (None: that of lagrange_dofmap, or max + 1 of a caller's cell_dofs2).  Every DOF of cell_dofs2 is written once,
    by its owner; other entries keep what `out` held (zeros if None)."""
    if p < 1 or p > 4:
        raise ValueError(f"prolong_lagrange: p = {p} outside 1 ... 4")
    pc = np.asarray(parent_cell, dtype=np.int64)
    uu = np.asarray(u, dtype=np.float64)
    one = uu.ndim == 1
    uu = uu.reshape(1, -1) if one else uu
    cd = lagrange_dofmap(mesh, p)[0] if cell_dofs is None else np.asarray(cell_dofs)
    if cell_dofs2 is None:
        cd2, n2 = lagrange_dofmap(mesh2, p)
    else:
        cd2 = np.asarray(cell_dofs2)
        n2 = int(cd2.max()) + 1
    ndofs2 = n2 if ndofs2 is None else int(ndofs2)
    ndofs = uu.shape[1] // bs
    cd, cd2 = cd.astype(np.int64), cd2.astype(np.int64)
    if cd.min() < 0 or cd.max() >= ndofs or cd2.min() < 0 or cd2.max() >= ndofs2:
        raise ValueError("prolong_lagrange: dofmap index out of range")
    rows = lattice_rows(p, child_vertex_positions(mesh, mesh2, pc, node_parent_facet))
    vP = np.moveaxis(uu.reshape(-1, ndofs, bs)[:, cd[pc]], 3, 1)     # [nrhs, bs, ncells2, nd]
    val, A = _contract(prolong_table(p), rows, vP)
    mask = dof_owners(mesh2, p)
    u2 = np.zeros((uu.shape[0], ndofs2 * bs)) if out is None else out.reshape(uu.shape[0], ndofs2 * bs)
    A2 = np.zeros_like(u2)
    for b in range(bs):
        u2[:, cd2[mask] * bs + b] = val[:, b][:, mask]
        A2[:, cd2[mask] * bs + b] = A[:, b][:, mask]
    if one:
        u2, A2 = u2[0], A2[0]
    return (u2, A2) if return_abs else u2


# ---- flux boundary conditions -------------------------------------------------------------------------------------
# The facet DOFs of local facet l of a cell are moments of the normal flux g (csrc/eqlb_boundary_update.hip):
#   DOF_j = pf_l sign(det J) |E| int_0^1 g(s) s^j ds,  pf_l = +1 for l = 1, -1 otherwise,
# s from the low local vertex va = (l == 0) ? 1 : 0 to vb = (l == 2) ? 1 : 2.  A boundary facet of the refined mesh is
# a whole parent facet or one of its halves, and a child keeps the orientation of its parent: with (a, b) the positions
# of the child's va, vb nodes on the parent facet (0: the parent's va node, 1: its vb node, 1/2: the bisecting node;
# node ids are matched, never coordinates), s = alpha + beta t, alpha = a, beta = b - a, and
#   dof2_j = sigma sum_i FB[m][j][i] dof_i,  sigma = pf_{l2} pf_l,  FB[m] = |beta| M H^{-1},
#   M[j][n] = int_0^1 (alpha + beta t)^n t^j dt,  H[j][i] = 1 / (i + j + 1)
# - the facet length cancels, no coordinates are read.  Every product is rounded on its own, the sum runs in ascending
# i, sigma is applied last.

FLUX_BC_MAPS = ((0, 2), (2, 0), (0, 1), (1, 2), (1, 0), (2, 1))   # (a, b) in half units, in the order of the table


def _solve_exact(A, B):
    """A^{-1} B in Fractions (Gauss-Jordan with the first non-zero pivot)."""
    n = len(A)
    M = [list(A[i]) + list(B[i]) for i in range(n)]
    for c in range(n):
        piv = next(r for r in range(c, n) if M[r][c] != 0)
        M[c], M[piv] = M[piv], M[c]
        M[c] = [v / M[c][c] for v in M[c]]
        for r in range(n):
            if r != c and M[r][c] != 0:
                M[r] = [v - M[r][c] * w for v, w in zip(M[r], M[c])]
    return [row[n:] for row in M]


@lru_cache(maxsize=None)
def flux_bc_table_exact(k):
    """FB [6][k][k] Fractions: the facet DOFs of a child facet from those of its parent, one matrix per map of
    FLUX_BC_MAPS."""
    if k < 1 or k > 4:
        raise ValueError(f"flux_bc_table: k = {k} outside 1 ... 4")
    from math import comb
    H = [[Fraction(1, i + j + 1) for i in range(k)] for j in range(k)]
    Hinv = _solve_exact(H, [[Fraction(int(i == j)) for j in range(k)] for i in range(k)])
    out = []
    for a2, b2 in FLUX_BC_MAPS:
        al, be = Fraction(a2, 2), Fraction(b2 - a2, 2)
        M = [[sum((comb(n, r) * al ** (n - r) * be ** r * Fraction(1, j + r + 1) for r in range(n + 1)), Fraction(0))
              for n in range(k)] for j in range(k)]
        out.append(tuple(tuple(abs(be) * sum((M[j][n] * Hinv[n][i] for n in range(k)), Fraction(0))
                               for i in range(k)) for j in range(k)))
    return tuple(out)


def flux_bc_table(k):
    """The table [6, k, k] as doubles, each entry rounded once."""
    return np.array([[[float(v) for v in row] for row in m] for m in flux_bc_table_exact(k)])


def flux_bc_maps(mesh, mesh2, parent_cell, node_parent_facet, facets2):
    """(cell2, l2, cell, l, m) of the listed boundary facets of the refined mesh: the one cell of the facet and its
    local index there, the parent cell and the local index of the parent facet there, the map of FLUX_BC_MAPS."""
    from .refine import parent_facets
    f2 = np.asarray(facets2, dtype=np.int64).ravel()
    nn = mesh.nnodes
    for i, f in enumerate(f2):
        if f < 0 or f >= mesh2.nfacets:
            raise ValueError(f"prolong_flux_bc: facets2[{i}] = {int(f)} is no facet of the refined mesh")
    cnt = np.diff(mesh2.facet_cells_offsets)[f2]
    if np.any(cnt != 1):
        i = int(np.nonzero(cnt != 1)[0][0])
        raise ValueError(f"prolong_flux_bc: facets2[{i}] = {int(f2[i])} lies between two cells")
    pf = parent_facets(mesh, node_parent_facet, mesh2).astype(np.int64)[f2]
    if np.any(pf < 0):
        i = int(np.nonzero(pf < 0)[0][0])
        raise ValueError(f"prolong_flux_bc: facets2[{i}] = {int(f2[i])} has no parent facet")
    npf = np.asarray(node_parent_facet, dtype=np.int64)
    C = mesh2.facet_cells[mesh2.facet_cells_offsets[f2]].astype(np.int64)
    P = np.asarray(parent_cell, dtype=np.int64)[C]
    hit2 = mesh2.cell_facets[C] == f2[:, None]
    hit = mesh.cell_facets[P] == pf[:, None]
    if not (np.all(hit2.sum(axis=1) == 1) and np.all(hit.sum(axis=1) == 1)):
        raise ValueError("prolong_flux_bc: the parent facet is no facet of the parent cell")
    l2, l = np.argmax(hit2, axis=1), np.argmax(hit, axis=1)
    va = lambda lf: np.where(lf == 0, 1, 0)   # noqa: E731  (the low local vertex first)
    vb = lambda lf: np.where(lf == 2, 1, 2)   # noqa: E731
    rows = np.arange(f2.size)
    w, v = mesh2.cell_nodes.astype(np.int64)[C], mesh.cell_nodes.astype(np.int64)[P]
    pa, pb = v[rows, va(l)], v[rows, vb(l)]

    def position(n):
        new = n >= nn
        mid = new & (npf[np.where(new, n - nn, 0)] == pf) if npf.size else np.zeros_like(new)
        return np.where(n == pa, 0, np.where(n == pb, 2, np.where(mid, 1, -1)))

    a, b = position(w[rows, va(l2)]), position(w[rows, vb(l2)])
    m = np.full(f2.size, -1, dtype=np.int64)
    for idx, (a2, b2) in enumerate(FLUX_BC_MAPS):
        m[(a == a2) & (b == b2)] = idx
    if np.any(m < 0):
        raise ValueError("prolong_flux_bc: a facet is neither its parent facet nor one of its halves")
    return C, l2, P, l, m


def apply_flux_bc_maps(k, m, dofs, sigma):
    """(val, A) [..., nlist, k]: sigma sum_i FB[m][j][i] dofs[..., i] and sum_i |FB| |dofs| for the maps m [nlist] and
    the signs sigma [nlist]; dofs [..., nlist, k].  Products rounded one by one, added in ascending i, sigma last."""
    T = flux_bc_table(k)[np.asarray(m, dtype=np.int64)]                 # [nlist, k, k]
    d = np.asarray(dofs, dtype=np.float64)
    val = T[..., 0] * d[..., None, 0]
    A = np.abs(T[..., 0]) * np.abs(d[..., None, 0])
    for i in range(1, k):
        val = val + T[..., i] * d[..., None, i]
        A = A + np.abs(T[..., i]) * np.abs(d[..., None, i])
    return np.asarray(sigma, dtype=np.float64)[:, None] * val, A


def prolong_flux_bc(mesh, mesh2, parent_cell, node_parent_facet, k, boundary_values, facets2, return_abs=False):
    """boundary_values [nrhs, ncells*k(k+2)] (the layout of eqlb_se_set_boundary; or 1-D) of the old mesh ->
    dofs [nrhs, nlist, k]: the facet DOFs of the boundary facets `facets2` of the refined mesh, each row in the form
    update_flux_bc takes without a rule.  return_abs: also A_j = sum_i |FB[m][j][i]| |dof_i|."""
    C, l2, P, l, m = flux_bc_maps(mesh, mesh2, parent_cell, node_parent_facet, facets2)
    nrt = k * (k + 2)
    bv = np.asarray(boundary_values, dtype=np.float64)
    one = bv.ndim == 1
    bv = bv.reshape(-1, mesh.ncells, nrt)
    d = bv[:, P[:, None], l[:, None] * k + np.arange(k)[None, :]]       # [nrhs, nlist, k]
    sigma = np.where(l2 == 1, 1.0, -1.0) * np.where(l == 1, 1.0, -1.0)
    val, A = apply_flux_bc_maps(k, m, d, sigma)
    if one:
        val, A = val[0], A[0]
    return (val, A) if return_abs else val


# ---- the transpose of the prolongation --------------------------------------------------------------------------------
# r = P^T r2 with P the matrix of prolong_lagrange, in a fixed order of operations: a store pass per coarse cell and
# the owner sum of the coarse level (csrc/eqlb_transfer.hip: k_restrict, then the sum pass of the coarse solver handle).
#   store pass  y_loc[c][i][b] = sum PT[row(k, n)][i] * r2[bs * dof2(c2, n) + b] over the children c2 = first + k of c in
#               ascending k and, within a child, over its local DOFs n in ascending n - only the DOFs the child OWNS
#               (dof_owners of the refined mesh: the rule by which prolong_lagrange stores, so every fine DOF is taken
#               exactly once); row(k, n) is the lattice row of prolong_lagrange.  Every product is rounded on its own and
#               the first term starts the sum; a cell whose children own nothing gives 0.0
#   owner sum   of the coarse level, as PoissonOperator.owner_sum of lsolver/primal.py, per component
#   mask        0 on the rows of `fixed` where given

def restrict_store_pass(mesh, mesh2, parent_cell, node_parent_facet, p, r2, bs=1):
    """(y_loc, A_loc) [ncells, nd_p, bs]: the store pass of restrict_lagrange and the same with absolute values."""
    if p < 1 or p > 4:
        raise ValueError(f"restrict_lagrange: p = {p} outside 1 ... 4")
    pc = np.asarray(parent_cell, dtype=np.int64)
    if pc.size != mesh2.ncells or np.any(np.diff(pc) < 0):
        raise ValueError("restrict_lagrange: the children of a cell are expected side by side, in the order of the cells")
    nd, nc = nd_of(p), mesh.ncells
    cd2, ndofs2 = lagrange_dofmap(mesh2, p)
    cd2 = cd2.astype(np.int64)
    rr = np.asarray(r2, dtype=np.float64).reshape(ndofs2, bs)
    rows = lattice_rows(p, child_vertex_positions(mesh, mesh2, pc, node_parent_facet))
    own = dof_owners(mesh2, p)
    T = prolong_table(p)
    first = np.searchsorted(pc, np.arange(nc), side="left")
    nchild = np.searchsorted(pc, np.arange(nc), side="right") - first
    y = np.zeros((nc, nd, bs))
    A = np.zeros((nc, nd, bs))
    started = np.zeros(nc, dtype=bool)
    for k in range(int(nchild.max())):
        for n in range(nd):
            c = np.nonzero(nchild > k)[0]
            c = c[own[first[c] + k, n]]
            if c.size == 0:
                continue
            c2 = first[c] + k
            term = T[rows[c2, n]][:, :, None] * rr[cd2[c2, n]][:, None, :]          # [sel, nd, bs]
            y[c] = np.where(started[c, None, None], y[c] + term, term)
            A[c] = A[c] + np.abs(term)
            started[c] = True
    return y, A


def restrict_lagrange(mesh, mesh2, parent_cell, node_parent_facet, p, r2, bs=1, fixed=None, return_abs=False, op=None):
    """r2 [ndofs2*bs] (read as r2[dof*bs + b]) of the P_p space on the refined mesh -> r = P^T r2 [ndofs*bs] on the old
    one, P the matrix of prolong_lagrange in the numbering of lagrange_dofmap; the order of operations stands in front
    of restrict_store_pass.  fixed [ndofs*bs] bool: these rows give 0.  return_abs: also the sum of the absolute values
    of the terms.  op: the operator of lsolver/primal.py on `mesh` whose slot lists the owner sum uses (None: a
    PoissonOperator(mesh, p) is built for it)."""
    from ..lsolver.primal import PoissonOperator
    y, A = restrict_store_pass(mesh, mesh2, parent_cell, node_parent_facet, p, r2, bs)
    if op is None:
        op = PoissonOperator(mesh, p)
    parts = [PoissonOperator.owner_sum(op, y[:, :, b]) for b in range(bs)]
    r = np.ascontiguousarray(np.stack(parts, axis=1).ravel())
    Ar = None
    if return_abs:
        Ar = np.ascontiguousarray(np.stack([PoissonOperator.owner_sum(op, A[:, :, b]) for b in range(bs)], axis=1).ravel())
    if fixed is not None:
        fx = np.asarray(fixed, dtype=bool).ravel()
        r[fx] = 0.0
        if return_abs:
            Ar[fx] = 0.0
    return (r, Ar) if return_abs else r
