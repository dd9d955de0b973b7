"""Shared by tests/test_multilevel_host.py and tests/test_gpu_multilevel.py: hierarchies of the numpy statements
(dolfinx_eqlb_amd/lsolver/multilevel.py) on meshes refined on the host, the prolongation as a dense matrix, and the
count of roundings behind the bound of the restriction."""

import numpy as np

import elasticity_cases as ec
import galerkin as gk
import primal_cases as pc
from dolfinx_eqlb_amd.lsolver import primal
from dolfinx_eqlb_amd.lsolver.multilevel import Hierarchy
from dolfinx_eqlb_amd.mesh import create_mesh
from dolfinx_eqlb_amd.mesh import transfer as tr
from dolfinx_eqlb_amd.mesh.refine import refine_longest_edge

U = pc.U


def refine_host(mesh, marked):
    """(mesh2, parent_cell, node_parent_facet) of the rule mesh.refine.refine_longest_edge"""
    x2, cells2, parent_cell, npf = refine_longest_edge(mesh, np.asarray(marked, dtype=np.int32))
    return create_mesh(x2, cells2), parent_cell, npf


def levels_host(base, marks):
    """meshes [L + 1] and links [L] = (parent_cell, node_parent_facet); marks[l](ncells) gives the cells of level l"""
    meshes, links = [base], []
    for mk in marks:
        m2, pcell, npf = refine_host(meshes[-1], mk(meshes[-1].ncells))
        meshes.append(m2)
        links.append((pcell, npf))
    return meshes, links


def all_cells(ncells):
    return np.arange(ncells, dtype=np.int32)


def coefficients(meshes, links, first):
    """a cell-wise coefficient per level: first(ncells) on the coarsest mesh, every child takes the value of its parent
    (the DG_0 prolongation an adaptive loop applies to its data)"""
    out = [first(meshes[0].ncells)]
    for pcell, _ in links:
        out.append(out[-1][np.asarray(pcell, dtype=np.int64)])
    return out


def poisson_op(mesh, p, kappa, facets=None):
    op = primal.PoissonOperator(mesh, p, kappa)
    op.set_dirichlet(mesh.boundary_facets() if facets is None else facets)
    return op


def elasticity_op(mesh, p, pi1, types=()):
    op = primal.ElasticityOperator(mesh, p, cell_pi1=pi1)
    op.set_dirichlet(*ec.dirichlet_lists(gk.elasticity_facet_types(mesh, list(types))))
    return op


def hierarchy(meshes, links, p, problem):
    """Hierarchy of "poisson" (kappa of primal_cases.kappa_of on the coarsest level) or "elasticity" (pi_1 of
    elasticity_cases.pi1_of) with Dirichlet conditions all around; also the coefficients per level"""
    if problem == "poisson":
        coeff = coefficients(meshes, links, pc.kappa_of)
        return Hierarchy([poisson_op(m, p, k) for m, k in zip(meshes, coeff)], links), coeff
    coeff = coefficients(meshes, links, ec.pi1_of)
    return Hierarchy([elasticity_op(m, p, k) for m, k in zip(meshes, coeff)], links), coeff


def dense_prolongation(mesh, mesh2, parent_cell, npf, p):
    """P [ndofs2, ndofs] by prolonging the identity: every entry is one table value (products with 0 and 1 are exact)"""
    n = tr.lagrange_dofmap(mesh, p)[1]
    return np.ascontiguousarray(tr.prolong_lagrange(mesh, mesh2, parent_cell, npf, p, np.eye(n)).T)


def check_restriction(mesh, mesh2, pcell, npf, p, bs, P=None, name=""):
    """mesh.transfer.restrict_lagrange of one link against the dense P^T (P: dense_prolongation of the link, built here
    where not given): the values and the abs-sum within restrict_terms, the pairing <P u, r2> = <u, R r2>, the mask.
    Returns max deviation / (2^-53 abs-sum) and the number of roundings allowed."""
    if P is None:
        P = dense_prolongation(mesh, mesh2, pcell, npf, p)
    n, n2 = P.shape[1], P.shape[0]
    rng = np.random.default_rng(10 * p + bs)
    r2 = rng.standard_normal(n2 * bs)
    r, A = tr.restrict_lagrange(mesh, mesh2, pcell, npf, p, r2, bs=bs, return_abs=True)
    ref = (P.T @ r2.reshape(n2, bs)).ravel()
    Aref = (np.abs(P).T @ np.abs(r2).reshape(n2, bs)).ravel()
    # the abs-sum of the statement is |P|^T |r2|, added in another order
    terms = sum(restrict_terms(mesh, p))
    assert np.all(np.abs(A - Aref) <= terms * U * Aref)
    dev = np.abs(r - ref)
    worst = float(np.max(dev / (U * Aref)))
    print(f"{name} p={p} bs={bs}: max deviation / (2^-53 abs-sum) {worst:.2f}, allowed {terms}".strip())
    assert np.all(dev <= terms * U * Aref)
    # the pairing <P u, r2> = <u, R r2>: the bound above per entry against |u|, the prolongation's own nd_p roundings per
    # entry against |r2|, and the two inner products
    u = rng.standard_normal(n * bs)
    Pu = tr.prolong_lagrange(mesh, mesh2, pcell, npf, p, u, bs=bs)
    lhs, rhs = np.sum(Pu * r2), np.sum(u * r)
    nd = (p + 1) * (p + 2) // 2
    assert abs(lhs - rhs) <= (terms + nd + (n + n2) * bs) * U * np.sum(np.abs(u) * Aref)
    # the mask
    fixed = rng.random(n * bs) < 0.3
    rm = tr.restrict_lagrange(mesh, mesh2, pcell, npf, p, r2, bs=bs, fixed=fixed)
    assert np.all(rm[fixed] == 0.0) and np.array_equal(rm[~fixed], r[~fixed])
    return worst, terms


def restrict_terms(mesh, p):
    """(statement, product): roundings along the longest chain of one entry of the restriction and of P^T r2 by a
    matrix product, each bounded by 2^-53 of the abs-sum |P|^T |r2|, in the way primal_cases.chain_terms counts.
    Statement: a coarse cell has at most 4 children of nd_p DOFs, one product and one addition per term: 4 nd_p; the
    owner sum: `valence`.  Product: a coarse DOF sees at most valence cells of 4 nd_p fine DOFs each."""
    nd = (p + 1) * (p + 2) // 2
    valence = int(np.diff(mesh.node_cells_offsets).max())
    return 4 * nd + valence, 4 * nd * valence
