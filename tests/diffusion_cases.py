"""Shared by the tests of the diffusion tensor (test_primal_diffusion_host.py, test_gpu_diffusion_bits.py,
test_gpu_diffusion_estimate.py, test_gpu_diffusion_chain.py): the tensors, the meshes, the stiffness matrix of
-div(kappa D grad u) assembled by quadrature as the independently rounded computation, and the rounding counts.  No test
lives here.

Tensors.  D = R(theta) diag(1, eps) R(theta)^T, eps in EPS: theta fixed (pi / 6), random per cell (seeded), and a two-layer
laminate (below the middle of the mesh diag(1, eps), above it the same rotated by pi / 3).  cell_D [ncells, 3] = (d00, d01,
d11).

Meshes.  sq12 = create_unit_square(12, shuffle_seed=3, perturb=0.15): 576 cells, three workgroups of the cell kernel, the
last one partial; aspect1000, tiny_far and triangle of primal_mesh_cases; the hierarchies of multilevel_cases through
primal_mesh_cases.levels_host.

Rounding counts.  chain_terms extends primal_cases.chain_terms by what the tensor adds to either chain: the statement
forms T = K D (two products, one sum: 3) in front of C = T K^T, which takes the place of K K^T at the same count; the
assembled side forms D grad phi_j (3) in front of the product with grad phi_i.  sig2_chain extends
estimator_cases.chain in the same way: W = adj(D) / (kappa det D) costs det D 2 (an accurate difference of products, within
2 units), kappa det D 1, the reciprocal 1 and the product with the entry of adj(D) 1, then W J (or W G_d) 3 - on the
kernel's side and on the statement's."""

import functools

import numpy as np
import scipy.sparse as sp

import estimator_cases as est
import primal_cases as pc
import primal_mesh_cases as pm
from dolfinx_eqlb_amd.elmtlib.lagrange import Lagrange
from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
from dolfinx_eqlb_amd.eqlb.check_eqlb_conditions import cell_geometry

import galerkin as gk

U = pc.U
EPS = (1.0, 1e-2, 1e-4)
KINDS = ("fixed", "random", "laminate")
MESHES = ("sq12", "aspect1000", "tiny_far", "triangle")
THETA = np.pi / 6
W_ROUNDINGS = 2 + 1 + 1 + 1      # det D, kappa det D, the reciprocal, the product with adj(D)


@functools.lru_cache(maxsize=None)
def mesh_of(name):
    if name == "sq12":
        from dolfinx_eqlb_amd.mesh import create_unit_square
        mesh = create_unit_square(12, shuffle_seed=3, perturb=0.15)
        assert (mesh.ncells, mesh.ncells // 256, mesh.ncells % 256) == (576, 2, 64)
        return mesh
    return pm.mesh_of(name)


def rotated(theta, eps):
    """(d00, d01, d11) of R(theta) diag(1, eps) R(theta)^T, arrays or numbers"""
    c, s = np.cos(theta), np.sin(theta)
    return np.stack(np.broadcast_arrays(c * c + eps * s * s, c * s * (1.0 - eps), s * s + eps * c * c), axis=-1)


def tensor_of(kind, mesh, eps, seed=17):
    """cell_D [ncells, 3]"""
    n = mesh.ncells
    if kind == "fixed":
        return np.ascontiguousarray(np.broadcast_to(rotated(THETA, eps), (n, 3)))
    if kind == "random":
        return np.ascontiguousarray(rotated(np.random.default_rng(seed).uniform(0.0, np.pi, n), eps))
    assert kind == "laminate"
    y = mesh.x[mesh.cell_nodes, 1].mean(axis=1)
    upper = y > 0.5 * (mesh.x[:, 1].min() + mesh.x[:, 1].max())
    return np.ascontiguousarray(rotated(np.where(upper, np.pi / 3, 0.0), eps))


def check_tensors():
    """what the table is there for"""
    mesh = mesh_of("sq12")
    for eps in EPS:
        for kind in KINDS:
            D = tensor_of(kind, mesh, eps)
            det = D[:, 0] * D[:, 2] - D[:, 1] ** 2
            assert D.shape == (mesh.ncells, 3) and np.all(D[:, 0] > 0) and np.all(det > 0)
            assert np.allclose(det, eps, rtol=1e-9) and np.allclose(D[:, 0] + D[:, 2], 1.0 + eps)
        lam = tensor_of("laminate", mesh, eps)
        assert 0 < (lam[:, 1] == 0.0).sum() < mesh.ncells or eps == 1.0
    assert np.unique(tensor_of("random", mesh, 1e-2)[:, 1]).size == mesh.ncells


def assemble(mesh, p, coeff, cell_D):
    """(A csr, |A|): int kappa (D grad phi_j) . grad phi_i by quadrature on physical gradients, in the numbering of
    galerkin.dofmap; |A| the same sum on the absolute values of every factor"""
    el = Lagrange(p)
    cd, ndofs = gk.dofmap(mesh, p)
    J, detJ, K = cell_geometry(mesh)
    qp, qw = make_quadrature_triangle(2 * p + 4)
    tab = el.tabulate(qp, 1)
    dphi = np.stack([tab[1], tab[2]], axis=2)
    g = np.einsum("cXd,qiX->cqid", K, dphi)
    D = np.asarray(cell_D).reshape(mesh.ncells, 3)
    Dm = np.stack([np.stack([D[:, 0], D[:, 1]], axis=1), np.stack([D[:, 1], D[:, 2]], axis=1)], axis=1)     # [c, 2, 2]
    kappa = np.ones(mesh.ncells) if coeff is None else np.asarray(coeff)
    w = qw[None, :] * (np.abs(detJ) * kappa)[:, None]
    dg, dga = np.einsum("cde,cqje->cqjd", Dm, g), np.einsum("cde,cqje->cqjd", np.abs(Dm), np.abs(g))
    Ke = np.einsum("cq,cqid,cqjd->cij", w, g, dg)
    Kabs = np.einsum("cq,cqid,cqjd->cij", w, np.abs(g), dga)
    nl = cd.shape[1]
    rows, cols = np.repeat(cd, nl, axis=1).ravel(), np.tile(cd, (1, nl)).ravel()
    return (sp.csr_matrix((Ke.ravel(), (rows, cols)), shape=(ndofs, ndofs)),
            sp.csr_matrix((Kabs.ravel(), (rows, cols)), shape=(ndofs, ndofs)))


def chain_terms(p, valence, nq):
    ts, ta = pc.chain_terms(p, valence, nq)
    return ts + 3, ta + 3


def sig2_chain(k, d, conforming):
    """roundings of cell_sig2 with the weight, the kernel's chain plus the statement's (the head of this file)"""
    c = est.chain("sig2_ev" if conforming else "sig2", k, d) + 2 * (W_ROUNDINGS + 3)
    return c + (2 * 3 if conforming else 0)


# ---- the chain of tests/test_gpu_diffusion_chain.py on the host ------------------------------------------------------------
# u = sin(pi x) sin(pi y) on the unit square, zero on the boundary, D = R(pi / 6) diag(1, eps) R^T constant, kappa = 1:
# f = -div(D grad u) = pi^2 ((d00 + d11) sin sin - 2 d01 cos cos)
CHAIN_N, CHAIN_THETA = 8, 0.5


def chain_mesh():
    from dolfinx_eqlb_amd.mesh import create_unit_square
    return create_unit_square(CHAIN_N)


def exact(eps):
    d00, d01, d11 = rotated(THETA, eps)
    pi = np.pi
    return dict(D=(d00, d01, d11),
                u=lambda x, y: np.sin(pi * x) * np.sin(pi * y),
                grad=lambda x, y: (pi * np.cos(pi * x) * np.sin(pi * y), pi * np.sin(pi * x) * np.cos(pi * y)),
                f=lambda x, y: pi * pi * ((d00 + d11) * np.sin(pi * x) * np.sin(pi * y)
                                          - 2.0 * d01 * np.cos(pi * x) * np.cos(pi * y)))


def points(mesh, qp):
    J = cell_geometry(mesh)[0]
    xq = mesh.x[mesh.cell_nodes[:, 0], :2][:, None, :] + np.einsum("cij,qj->cqi", J, qp)
    return xq[..., 0], xq[..., 1]


def energy_error2(mesh, p, u, cd, eps, cell_D):
    """|| D^(1/2) grad(u - u_h) ||^2 by a quadrature of degree 2 p + 6 on the host"""
    ex = exact(eps)
    qp, qw = make_quadrature_triangle(2 * p + 6)
    J, detJ, K = cell_geometry(mesh)
    tab = Lagrange(p).tabulate(qp, 1)
    gh = np.einsum("cXd,qiX,ci->cqd", K, np.stack([tab[1], tab[2]], axis=2), u[cd])
    xq, yq = points(mesh, qp)
    gx, gy = ex["grad"](xq, yq)
    e0, e1 = gx - gh[..., 0], gy - gh[..., 1]
    D = np.asarray(cell_D).reshape(-1, 3)
    q = D[:, 0, None] * e0 * e0 + 2.0 * D[:, 1, None] * e0 * e1 + D[:, 2, None] * e1 * e1
    return float(np.sum(qw[None, :] * np.abs(detJ)[:, None] * q))


def host_level(oracle, mesh, k, eps, cell_D):
    """One level of the chain by the statements: the Galerkin solution of the matrix assembled by quadrature (sparse
    direct solve), flux_dg_tensor, the oracle's equilibration, weighted_flux_norm, the oscillation with the weight
    1 / sqrt(lambda_min) - and the unweighted flux norm beside it.  Returns the cell-wise terms and the error."""
    import scipy.sparse.linalg as spla
    import sys
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from gen_tables import primal_table_float
    from synthetic import facet_types
    from dolfinx_eqlb_amd.eqlb import check_eqlb_conditions as chk
    from dolfinx_eqlb_amd.lsolver import primal
    ex = exact(eps)
    op = primal.PoissonOperator(mesh, k)
    op.set_dirichlet(mesh.boundary_facets())
    op.set_diffusion(cell_D)
    qp, qw = make_quadrature_triangle(2 * k + 6)
    xq, yq = points(mesh, qp)
    fv = ex["f"](xq, yq)
    psi = Lagrange(k - 1).tabulate(qp)[0]
    Md = np.einsum("q,qn,qm->nm", qw, psi, psi)
    fh = np.linalg.solve(Md, np.einsum("q,qn,cq->nc", qw, psi, fv)).T.ravel()         # the L2 projection of f into DG_{k-1}
    b = op.load(k - 1, fh)
    A = assemble(mesh, k, None, cell_D)[0].tocsr()
    free = np.nonzero(~op.fixed)[0]
    u = np.zeros(op.ndofs)
    u[free] = spla.spsolve(A[free][:, free].tocsc(), b[free])
    cd = op.cell_dofs
    G = primal.flux_dg_tensor(mesh, k, k - 1, cd, u, cell_D, primal_table_float(k, k - 1))[0]
    x = oracle.se_reconstruct(mesh, k, facet_types(mesh, None), G[None], fh[None])[0]
    sig2 = chk.weighted_flux_norm(mesh, k, x, G, k - 1, None, cell_D)
    plain = chk.weighted_flux_norm(mesh, k, x, G, k - 1, None, None)
    osc = chk.oscillation_term(mesh, k, x, G, ex["f"], 2 * k + 6, primal.diffusion_oscillation_weight(cell_D))
    return dict(u=u, cd=cd, fh=fh, fv=fv, G=G, x=x, sig2=sig2, plain=plain, osc=osc, qp=qp, qw=qw,
                err2=energy_error2(mesh, k, u, cd, eps, cell_D))


def eta2_of(sig2, osc):
    """cell-wise (sqrt sig2 + sqrt osc)^2"""
    return (np.sqrt(sig2) + np.sqrt(osc)) ** 2
