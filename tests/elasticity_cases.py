"""Shared by tests/test_primal_elasticity_host.py, tests/test_primal_meshes_host.py and
tests/test_gpu_primal_elasticity.py: the Galerkin matrix and load of the P_p^2 elasticity problem -div(2 eps(u) + pi_1 div(u) I) = f assembled the way galerkin.solve_elasticity builds
its cell matrices (quadrature on physical gradients, scipy), with pi_1 in front of the div-div term, in the blocked
numbering x[2 dof + r]: the independently rounded computation the statement of dolfinx_eqlb_amd/lsolver/primal.py
(ElasticityOperator) is compared with, and that comparison itself (check_statement)."""

import numpy as np
import scipy.sparse as sp

from dolfinx_eqlb_amd.elmtlib.lagrange import Lagrange
from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
from dolfinx_eqlb_amd.eqlb.check_eqlb_conditions import cell_geometry

import galerkin as gk

U = 2.0 ** -53


def assemble(mesh, p, pi_1=1.0, cell_pi1=None, degree_dg=None, rhs_dg=None):
    """(A csr [2 ndofs, 2 ndofs], |A| (the same sum with the absolute values of the quadrature terms), b, |b|) in the
    blocked numbering 2 dof + r of galerkin.dofmap (that of mesh.transfer.lagrange_dofmap); rhs_dg [2][ncells * nd_d]."""
    el = Lagrange(p)
    cd, ndofs = gk.dofmap(mesh, p)
    J, detJ, K = cell_geometry(mesh)
    qp, qw = make_quadrature_triangle(2 * p + 4)
    tab = el.tabulate(qp, 1)
    dphi = np.stack([tab[1], tab[2]], axis=2)
    g = np.einsum("cXd,qiX->cqid", K, dphi)                  # [c, q, i, d] physical gradients
    pi = np.full(mesh.ncells, float(pi_1)) if cell_pi1 is None else np.asarray(cell_pi1, dtype=np.float64)
    w = qw[None, :] * np.abs(detJ)[:, None]
    nl = cd.shape[1]

    def cell_matrices(g, pi):
        gg = np.einsum("cq,cqid,cqjd->cij", w, g, g)
        gx = np.einsum("cq,cqir,cqjs->cirjs", w, g, g)       # d_r phi_i d_s phi_j
        Ke = np.zeros((mesh.ncells, nl, 2, nl, 2))
        for r in range(2):
            Ke[:, :, r, :, r] += gg
        Ke += np.einsum("cirjs->cisjr", gx)                  # d_s phi_i d_r phi_j  (grad u^T term)
        Ke += pi[:, None, None, None, None] * gx             # pi_1 div u div v
        return Ke.reshape(mesh.ncells, 2 * nl, 2 * nl)

    vd = (2 * cd[:, :, None] + np.arange(2)[None, None, :]).reshape(mesh.ncells, 2 * nl)
    rows, cols = np.repeat(vd, 2 * nl, axis=1).ravel(), np.tile(vd, (1, 2 * nl)).ravel()
    A = sp.csr_matrix((cell_matrices(g, pi).ravel(), (rows, cols)), shape=(2 * ndofs, 2 * ndofs))
    Aabs = sp.csr_matrix((cell_matrices(np.abs(g), np.abs(pi)).ravel(), (rows, cols)), shape=(2 * ndofs, 2 * ndofs))
    b = babs = None
    if rhs_dg is not None:
        psi = Lagrange(degree_dg).tabulate(qp)[0]
        f = np.asarray(rhs_dg).reshape(2, mesh.ncells, -1)
        b, babs = np.zeros(2 * ndofs), np.zeros(2 * ndofs)
        for r in range(2):
            fe = np.einsum("cq,cn,qn,qi->ci", w, f[r], psi, tab[0])
            fa = np.einsum("cq,cn,qn,qi->ci", w, np.abs(f[r]), np.abs(psi), np.abs(tab[0]))
            np.add.at(b, (2 * cd + r).ravel(), fe.ravel())
            np.add.at(babs, (2 * cd + r).ravel(), fa.ravel())
    return A, Aabs, b, babs


def chain_terms(p, valence, nq):
    """(statement, assembled): roundings along the longest chain of either computation of one entry of A u, each bounded
    by 2^-53 of that computation's OWN abs-sum, as primal_cases.chain_terms counts them for the Poisson problem.
    Statement: geometry 20 (an entry of J 1; det = two products of entries and a difference 4; idet 5; K = J idet 7;
    Q = K K 15; the factor |det| and its product 5), contraction nd_p, the combination D_ab 3 (a product and two sums),
    the sums of y_loc 5 (two levels of sums, the product with pi_c and its sum, the last sum), owner sum `valence`.
    Assembled: points, weights and monomial powers of the tabulation 2 (p + 3), geometry 12, the products and the sum of
    the quadrature nq + 4, the three terms of an entry (two sums, the product with pi_c) 3, the sum over the cells
    `valence`, the product with u 2 nd_p * valence (a row meets both components of every DOF of its cells)."""
    nd = (p + 1) * (p + 2) // 2
    return 20 + nd + 3 + 5 + valence, 2 * (p + 3) + 12 + nq + 4 + 3 + valence + 2 * nd * valence


def pi1_of(ncells, seed=23):
    """log-uniform in [0.5, 50] per cell"""
    return 0.5 * 100.0 ** np.random.default_rng(seed).random(ncells)


def dirichlet_lists(ft):
    """the two facet lists of set_dirichlet from facet types [2, nfacets]: the facets with ft[r] == 1"""
    return [np.nonzero(ft[r] == 1)[0].astype(np.int32) for r in range(2)]


def check_statement(mesh, p, per_cell, name=""):
    """The statement (lsolver.primal.ElasticityOperator) against the assembled operator on one mesh, with the scalar
    pi_1 = 3.5 or the per-cell pi_1 of pi1_of: apply, load and diagonal within chain_terms of the mesh's own valence,
    b_extra added as it is, residual and mask (Dirichlet all around in both rows).  Returns the largest |diff| / bound
    of (apply, load, diagonal)."""
    from dolfinx_eqlb_amd.lsolver import primal
    from primal_cases import ratio
    rng = np.random.default_rng(5 + p)
    pi_1, cell_pi1 = (1.0, pi1_of(mesh.ncells)) if per_cell else (3.5, None)
    op = primal.ElasticityOperator(mesh, p, pi_1, cell_pi1)
    d = min(p - 1, 3) if p > 1 else 1
    nd = (d + 1) * (d + 2) // 2
    f = rng.standard_normal((2, mesh.ncells * nd))
    A, Aabs, b, babs = assemble(mesh, p, pi_1, cell_pi1, d, f)
    assert A.shape[0] == 2 * op.ndofs
    u = rng.standard_normal(2 * op.ndofs)
    valence = int(np.diff(mesh.node_cells_offsets).max())
    ts, ta = chain_terms(p, valence, make_quadrature_triangle(2 * p + 4)[1].size)
    label = f"{name} p={p} per_cell={per_cell}".strip()
    ratios = []
    # operator
    y, yabs = op.apply(u, return_abs=True)
    diff, bound = np.abs(y - A @ u), U * (ts * yabs + ta * (Aabs @ np.abs(u)))
    ratios.append(ratio(diff, bound))
    print(f"{label}: apply max |diff| / bound = {ratios[-1]:.3f} (terms {(ts, ta)})")
    assert np.all(diff <= bound)
    # load (b_extra is added as it is)
    e = rng.standard_normal(2 * op.ndofs)
    bs, bsabs = op.load(d, f, return_abs=True)
    diff, bound = np.abs(bs - b), U * (ts * bsabs + ta * babs)
    ratios.append(ratio(diff, bound))
    print(f"{label}: load max |diff| / bound = {ratios[-1]:.3f}")
    assert np.all(diff <= bound)
    assert np.array_equal(op.load(d, f, e), bs + e)
    # diagonal
    dg, dabs = op.diagonal(return_abs=True)
    diff, bound = np.abs(dg - A.diagonal()), U * (ts * dabs + ta * Aabs.diagonal())
    ratios.append(ratio(diff, bound))
    print(f"{label}: diagonal max |diff| / bound = {ratios[-1]:.3f}")
    assert np.all(diff <= bound) and np.all(dg > 0.0)
    # residual and mask
    bf = mesh.boundary_facets()
    op.set_dirichlet(bf, bf)
    r = op.residual(bs, u)
    assert np.array_equal(r[~op.fixed], (bs - y)[~op.fixed]) and np.all(r[op.fixed] == 0.0)
    ym = op.apply(u, masked=True)
    assert np.array_equal(ym[~op.fixed], y[~op.fixed]) and np.all(ym[op.fixed] == 0.0)
    return tuple(ratios)
