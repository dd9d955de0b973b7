"""Shared by tests/test_primal_reaction_host.py and the tests/test_gpu_reaction_*.py files: the reaction coefficient of
the cases, the quadrature mass matrix assembled beside primal_cases.assemble (the independently rounded computation the
reaction term of dolfinx_eqlb_amd/lsolver/primal.py is compared with) and the chain counts with the roundings the term
adds.  No test lives here."""

import numpy as np
import scipy.sparse as sp

from dolfinx_eqlb_amd.elmtlib.lagrange import Lagrange
from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
from dolfinx_eqlb_amd.eqlb.check_eqlb_conditions import cell_geometry

import elasticity_cases as ec
import galerkin as gk
import primal_cases as pc

U = pc.U
STATEMENT_MESHES = ("base9", "disk100", "tiny_far", "aspect1000")
BIT_MESHES = ("disk100", "hole", "delaunay", "tiny_far", "huge", "aspect1000", "wg128", "wg256", "triangle", "right1")


def mesh_of(name):
    """base9 is the base mesh of tests/test_gpu_primal_solve.py; the others are those of primal_mesh_cases"""
    if name == "base9":
        from dolfinx_eqlb_amd.mesh import create_unit_square
        mesh = create_unit_square(9, shuffle_seed=3, perturb=0.15)
        assert mesh.ncells == 324
        return mesh
    import primal_mesh_cases as pm
    return pm.mesh_of(name)


def c_of(ncells, seed=31, lo=-2.0, hi=4.0):
    """cell-wise c: log-uniform in [1e-2, 1e4], every seventh cell exactly 0"""
    c = 10.0 ** (lo + (hi - lo) * np.random.default_rng(seed).random(ncells))
    c[::7] = 0.0
    return c


def assemble_mass(mesh, p, c, bs=1):
    """(M csr, |M|): sum_q w_q c_T |det J| phi_i(X_q) phi_j(X_q) with the quadrature of primal_cases.assemble, and the
    same sum with absolute values; bs = 2: block diagonal in the blocked numbering 2 dof + r."""
    cd, ndofs = gk.dofmap(mesh, p)
    _, detJ, _ = cell_geometry(mesh)
    qp, qw = make_quadrature_triangle(2 * p + 4)
    phi = Lagrange(p).tabulate(qp)[0]
    w = qw[None, :] * (np.abs(detJ) * np.asarray(c, dtype=np.float64))[:, None]
    Me = np.einsum("cq,qi,qj->cij", w, phi, phi)
    Ma = np.einsum("cq,qi,qj->cij", w, np.abs(phi), np.abs(phi))
    nl = cd.shape[1]
    rows, cols = np.repeat(cd, nl, axis=1).ravel(), np.tile(cd, (1, nl)).ravel()
    M = sp.csr_matrix((Me.ravel(), (rows, cols)), shape=(ndofs, ndofs))
    Mabs = sp.csr_matrix((Ma.ravel(), (rows, cols)), shape=(ndofs, ndofs))
    if bs == 2:
        M, Mabs = sp.kron(M, sp.identity(2)).tocsr(), sp.kron(Mabs, sp.identity(2)).tocsr()
    return M, Mabs


def chain_terms(problem, p, valence, nq):
    """(statement, assembled) of primal_cases.chain_terms / elasticity_cases.chain_terms with the roundings the reaction
    term adds to the longest chain of one entry of A u.
    Statement: the value without the term is formed as before and then takes ONE more addition, + wm m[i]: + 1.  The
    chain through the new term itself is shorter than the one it joins (|det| 4, wm = c_T |det| 1, the contraction nd_p,
    the product wm m 1, that addition 1, the owner sum: nd_p + 7 + valence against 12 + nd_p + 5 + valence + 1), so it
    does not count.
    Assembled: (A u) + (M u) is one more addition, + 1; the chain through M (tabulation 2 (p + 3), |det| and c_T 5, the
    products and the sum of the quadrature nq + 4, the cells, the product with u) is no longer than that through A."""
    ts, ta = (pc if problem == "poisson" else ec).chain_terms(p, valence, nq)
    return ts + 1, ta + 1


def assembled(problem, mesh, p, coeff, c):
    """stiffness + mass of the cases, csr"""
    import primal_mesh_cases as pm
    return (pm.assembled(problem, mesh, p, coeff) + assemble_mass(mesh, p, c, 1 if problem == "poisson" else 2)[0]).tocsr()
