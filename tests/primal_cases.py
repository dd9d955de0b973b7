"""Shared by tests/test_primal_host.py and tests/test_gpu_primal_solve.py: the Galerkin matrix and load of the P_p
Poisson problem assembled the way tests/galerkin.py assembles them (quadrature on physical gradients, scipy), as the
independently rounded computation the statement of dolfinx_eqlb_amd/lsolver/primal.py is compared with."""

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
