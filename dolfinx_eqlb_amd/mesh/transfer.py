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
