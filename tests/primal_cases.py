"""Shared by tests/test_primal_host.py, tests/test_primal_meshes_host.py and tests/test_gpu_primal_solve.py: the Galerkin
matrix and load of the P_p Poisson problem assembled the way tests/galerkin.py assembles them (quadrature on physical
gradients, scipy), as the independently rounded computation the statement of dolfinx_eqlb_amd/lsolver/primal.py is
compared with, and that comparison itself (check_statement)."""

import numpy as np
import scipy.sparse as sp

from dolfinx_eqlb_amd.elmtlib.lagrange import Lagrange
from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
from dolfinx_eqlb_amd.eqlb.check_eqlb_conditions import cell_geometry

import galerkin as gk

U = 2.0 ** -53


def assemble(mesh, p, coeff=None, degree_dg=None, rhs_dg=None):
    """(A csr [ndofs, ndofs], |A| (the same sum with the absolute values of the quadrature terms), b, |b|) in the
    numbering of galerkin.dofmap, which is that of mesh.transfer.lagrange_dofmap."""
    el = Lagrange(p)
    cd, ndofs = gk.dofmap(mesh, p)
    J, detJ, K = cell_geometry(mesh)
    qp, qw = make_quadrature_triangle(2 * p + 4)
    tab = el.tabulate(qp, 1)
    dphi = np.stack([tab[1], tab[2]], axis=2)
    g = np.einsum("cXd,qiX->cqid", K, dphi)
    kappa = np.ones(mesh.ncells) if coeff is None else np.asarray(coeff)
    w = qw[None, :] * (np.abs(detJ) * kappa)[:, None]
    Ke = np.einsum("cq,cqid,cqjd->cij", w, g, g)
    Kabs = np.einsum("cq,cqid,cqjd->cij", w, np.abs(g), np.abs(g))
    nl = cd.shape[1]
    rows, cols = np.repeat(cd, nl, axis=1).ravel(), np.tile(cd, (1, nl)).ravel()
    A = sp.csr_matrix((Ke.ravel(), (rows, cols)), shape=(ndofs, ndofs))
    Aabs = sp.csr_matrix((Kabs.ravel(), (rows, cols)), shape=(ndofs, ndofs))
    b = babs = None
    if rhs_dg is not None:
        psi = Lagrange(degree_dg).tabulate(qp)[0]
        f = np.asarray(rhs_dg).reshape(mesh.ncells, -1)
        wd = qw[None, :] * np.abs(detJ)[:, None]
        fe = np.einsum("cq,cn,qn,qi->ci", wd, f, psi, tab[0])
        fa = np.einsum("cq,cn,qn,qi->ci", wd, np.abs(f), np.abs(psi), np.abs(tab[0]))
        b, babs = np.zeros(ndofs), np.zeros(ndofs)
        np.add.at(b, cd.ravel(), fe.ravel())
        np.add.at(babs, cd.ravel(), fa.ravel())
    return A, Aabs, b, babs


def chain_terms(p, valence, nq):
    """(statement, assembled): roundings along the longest chain of either computation of one entry of A u, each bounded
    by 2^-53 of that computation's OWN abs-sum (the statement's abs-sum knows the exact integrals |S[i][j]|, |Load[i][n]|
    only: the cancellation inside a quadrature sum shows in the assembled abs-sum alone).  Statement: geometry 12,
    contraction nd_p, combination 5, owner sum `valence`.  Assembled: points, weights and monomial powers of the
    tabulation 2 (p + 3), geometry 12, the products and the sum of the quadrature nq + 4, the sum over the cells
    `valence`, the product with u nd_p * valence."""
    nd = (p + 1) * (p + 2) // 2
    return 12 + nd + 5 + valence, 2 * (p + 3) + 12 + nq + 4 + valence + nd * valence


def kappa_of(ncells, seed=11):
    """log-uniform in [1, 100] per cell"""
    return 10.0 ** (2.0 * np.random.default_rng(seed).random(ncells))


def ratio(diff, bound):
    """max of diff / bound with 0 / 0 = 0 (printed); the assertion is diff <= bound entry by entry"""
    return float(np.max(np.where(bound > 0.0, diff / np.where(bound > 0.0, bound, 1.0), np.where(diff > 0.0, np.inf, 0.0))))


def check_statement(mesh, p, name):
    """The statement (lsolver.primal.PoissonOperator) against the assembled operator on one mesh: apply, load and
    diagonal within chain_terms of the mesh's own valence, b_extra added as it is, residual and mask.  Returns the
    largest |diff| / bound of (apply, load, diagonal)."""
    from dolfinx_eqlb_amd.lsolver import primal
    rng = np.random.default_rng(5 + p)
    kappa = kappa_of(mesh.ncells)
    op = primal.PoissonOperator(mesh, p, kappa)
    d = min(p - 1, 3) if p > 1 else 1
    nd = (d + 1) * (d + 2) // 2
    f = rng.standard_normal(mesh.ncells * nd)
    A, Aabs, b, babs = assemble(mesh, p, kappa, d, f)
    assert A.shape[0] == op.ndofs
    u = rng.standard_normal(op.ndofs)
    valence = int(np.diff(mesh.node_cells_offsets).max())
    ts, ta = chain_terms(p, valence, make_quadrature_triangle(2 * p + 4)[1].size)
    terms = (ts, ta)
    ratios = []
    # operator
    y, yabs = op.apply(u, return_abs=True)
    diff, bound = np.abs(y - A @ u), U * (ts * yabs + ta * (Aabs @ np.abs(u)))
    ratios.append(ratio(diff, bound))
    print(f"{name} p={p}: apply max |diff| / bound = {ratios[-1]:.3f} (terms {terms})")
    assert np.all(diff <= bound)
    # load (b_extra is added as it is)
    e = rng.standard_normal(op.ndofs)
    bs, bsabs = op.load(d, f, return_abs=True)
    diff, bound = np.abs(bs - b), U * (ts * bsabs + ta * babs)
    ratios.append(ratio(diff, bound))
    print(f"{name} p={p}: load max |diff| / bound = {ratios[-1]:.3f}")
    assert np.all(diff <= bound)
    assert np.array_equal(op.load(d, f, e), bs + e)
    # diagonal
    dg, dabs = op.diagonal(return_abs=True)
    diff, bound = np.abs(dg - A.diagonal()), U * (ts * dabs + ta * Aabs.diagonal())
    ratios.append(ratio(diff, bound))
    print(f"{name} p={p}: diagonal max |diff| / bound = {ratios[-1]:.3f}")
    assert np.all(diff <= bound) and np.all(dg > 0.0)
    # residual and mask
    op.set_dirichlet(mesh.boundary_facets())
    r = op.residual(bs, u)
    assert np.array_equal(r[~op.fixed], (bs - y)[~op.fixed]) and np.all(r[op.fixed] == 0.0)
    ym = op.apply(u, masked=True)
    assert np.array_equal(ym[~op.fixed], y[~op.fixed]) and np.all(ym[op.fixed] == 0.0)
    assert op.fixed.sum() == np.unique(mesh.facet_nodes[mesh.boundary_facets()]).size \
        + (p - 1) * mesh.boundary_facets().size
    return tuple(ratios)
