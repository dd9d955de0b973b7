"""Shared by tests/test_primal_robin_host.py and the tests/test_gpu_*robin*.py files: the Robin lists of the cases, the
boundary mass assembled by quadrature (the independently rounded computation the Robin term of dolfinx_eqlb_amd/lsolver/
primal.py is compared with), and the model problem of the chains.  No test lives here.

The model problem: u = sin(omega x) sin(pi y) on the unit square with tan(omega) = -omega / alpha, alpha = 1, so that
-du/dn = alpha u on x = 1 (u_ext = 0) and u = 0 on the other three sides; f = (omega^2 + pi^2) u.  The energy norm is
|||e|||^2 = || grad e ||^2 + || alpha^(1/2) e ||^2 on the Robin side."""

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import galerkin as gk
import primal_cases as pc
from dolfinx_eqlb_amd.elmtlib.lagrange import Lagrange
from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_interval
from dolfinx_eqlb_amd.eqlb.bcs import _facet_points

U = pc.U
ALPHA = 1.0


def _omega(alpha):
    lo, hi = 0.5 * np.pi + 1e-12, np.pi          # tan(w) + w / alpha rises from -inf to pi / alpha
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if np.tan(mid) + mid / alpha < 0.0:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


OMEGA = _omega(ALPHA)


def u_ex(x, y):
    return np.sin(OMEGA * x) * np.sin(np.pi * y)


def grad_ex(x, y):
    return OMEGA * np.cos(OMEGA * x) * np.sin(np.pi * y), np.pi * np.sin(OMEGA * x) * np.cos(np.pi * y)


def f_ex(x, y):
    return (OMEGA ** 2 + np.pi ** 2) * u_ex(x, y)


def chain_mesh(n):
    from dolfinx_eqlb_amd.mesh import create_unit_square
    return create_unit_square(n, shuffle_seed=3, perturb=0.15)


def sides(mesh):
    """the boundary facets of x = 0, y = 0, x = 1, y = 1 of a unit square (int32, ascending)"""
    bf = mesh.boundary_facets()
    mp = mesh.facet_midpoints()[bf]
    tests = (np.abs(mp[:, 0]) < 1e-9, np.abs(mp[:, 1]) < 1e-9, np.abs(mp[:, 0] - 1) < 1e-9, np.abs(mp[:, 1] - 1) < 1e-9)
    out = [bf[t].astype(np.int32) for t in tests]
    assert sum(o.size for o in out) == bf.size
    return out


def alpha_of(n, seed=17):
    """facet-wise alpha in [0, 10], every fifth one exactly 0"""
    a = 10.0 * np.random.default_rng(seed).random(n)
    a[::5] = 0.0
    return a


def facet_geometry(mesh, facets):
    facets = np.asarray(facets, dtype=np.int64)
    cells = mesh.facet_cells[mesh.facet_cells_offsets[facets]]
    lf = np.argmax(mesh.cell_facets[cells] == facets[:, None], axis=1)
    return cells, lf


def assemble_boundary_mass(mesh, p, facets, alpha):
    """(B csr, |B|): sum_q w_q alpha_f |E_f| phi_i(X_q) phi_j(X_q) over the listed boundary facets, phi the basis of
    the facet's one cell at the points of the facet (a Gauss rule of degree 2 p + 2: exact), in the numbering of
    galerkin.dofmap - it knows nothing of the local order of a facet's rows."""
    cd, ndofs = gk.dofmap(mesh, p)
    facets = np.asarray(facets, dtype=np.int64)
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), facets.shape)
    cells, lf = facet_geometry(mesh, facets)
    s, wq = make_quadrature_interval(2 * p + 2)
    pts = _facet_points(s)
    phi = np.stack([Lagrange(p).tabulate(pts[l])[0] for l in range(3)])          # [3, nq, nd]
    X = mesh.x[mesh.cell_nodes[cells], :2]
    i = np.arange(facets.size)
    va, vb = np.where(lf == 0, 1, 0), np.where(lf == 2, 1, 2)
    E = np.linalg.norm(X[i, vb] - X[i, va], axis=1)
    w = (alpha * E)[:, None] * wq[None, :]
    Be = np.einsum("fq,fqi,fqj->fij", w, phi[lf], phi[lf])
    Ba = np.einsum("fq,fqi,fqj->fij", w, np.abs(phi[lf]), np.abs(phi[lf]))
    nl = cd.shape[1]
    rows, cols = np.repeat(cd[cells], nl, axis=1).ravel(), np.tile(cd[cells], (1, nl)).ravel()
    return (sp.csr_matrix((Be.ravel(), (rows, cols)), shape=(ndofs, ndofs)),
            sp.csr_matrix((Ba.ravel(), (rows, cols)), shape=(ndofs, ndofs)))


def trace_values(mesh, p, facets, u, s):
    """u_h at the facet parameters s (the frame of eqlb_facet_points) of the listed boundary facets, [n, nq], from the
    basis of the facet's cell: independent of the facet-local order of lsolver.primal.robin_flux"""
    cd, _ = gk.dofmap(mesh, p)
    cells, lf = facet_geometry(mesh, facets)
    pts = _facet_points(np.asarray(s, dtype=np.float64))
    phi = np.stack([Lagrange(p).tabulate(pts[l])[0] for l in range(3)])
    return np.einsum("fqi,fi->fq", phi[lf], np.asarray(u)[cd[cells]])


def boundary_error2(mesh, p, facets, alpha, u):
    """int alpha (u - u_h)^2 over the listed facets (Gauss rule of degree 2 p + 6)"""
    from dolfinx_eqlb_amd.eqlb.check_eqlb_conditions import cell_geometry
    facets = np.asarray(facets, dtype=np.int64)
    cells, lf = facet_geometry(mesh, facets)
    s, wq = make_quadrature_interval(2 * p + 6)
    uh = trace_values(mesh, p, facets, u, s)
    J = cell_geometry(mesh)[0]
    pts = _facet_points(s)
    xq = mesh.x[mesh.cell_nodes[cells, 0], :2][:, None, :] + np.einsum("cij,cqj->cqi", J[cells], pts[lf])
    X = mesh.x[mesh.cell_nodes[cells], :2]
    i = np.arange(facets.size)
    va, vb = np.where(lf == 0, 1, 0), np.where(lf == 2, 1, 2)
    E = np.linalg.norm(X[i, vb] - X[i, va], axis=1)
    a = np.broadcast_to(np.asarray(alpha, dtype=np.float64), facets.shape)
    return float(np.sum((a * E)[:, None] * wq[None, :] * (u_ex(xq[..., 0], xq[..., 1]) - uh) ** 2))


def flux_rule(k):
    """the rule of the moments of the flux condition: Gauss, exact for degree 2 k + 2 on [0, 1]"""
    return make_quadrature_interval(2 * k + 2)


def galerkin_level(mesh, k, fh):
    """The Galerkin solution of the model problem's boundary layout on `mesh` for the DG_{k-1} right-hand side fh (sparse
    direct solve of the matrix assembled by quadrature with the boundary mass): dict(u, G, ft, right, dirichlet)."""
    left, bottom, right, top = sides(mesh)
    A, _, b, _ = pc.assemble(mesh, k, None, k - 1, fh)
    B, _ = assemble_boundary_mass(mesh, k, right, ALPHA)
    cd, ndofs = gk.dofmap(mesh, k)
    dir_f = np.concatenate([left, bottom, top])
    fixed = np.zeros(ndofs, dtype=bool)
    fixed[mesh.facet_nodes[dir_f].ravel()] = True
    for j in range(k - 1):
        fixed[mesh.nnodes + dir_f * (k - 1) + j] = True
    free = np.nonzero(~fixed)[0]
    u = np.zeros(ndofs)
    u[free] = spla.spsolve((A + B).tocsr()[free][:, free].tocsc(), b[free])
    G = gk.discrete_flux(mesh, k, u, cd)
    ft = np.zeros((1, mesh.nfacets), dtype=np.int8)
    ft[0, mesh.boundary_facets()] = 1
    ft[0, right] = 2
    return dict(u=u, G=G, ft=ft, right=right, dirichlet=dir_f, cd=cd)


def host_level(oracle_mod, mesh, k, robin_flux=True):
    """One level of the host chain on `mesh`: the Galerkin solve with the boundary mass (sparse direct), the oracle with
    boundary_values = the moments of alpha u_h on the Robin side (robin_flux=False: a zero flux prescribed there), the
    estimator.  Returns dict(u, G, fh, ft, bv, x, sig2, osc, eta2, err2, div_res)."""
    from test_gpu_bc_update import dense_table, numpy_dofs
    from test_gpu_estimate import flux_norm2_cells
    from dolfinx_eqlb_amd.eqlb import check_eqlb_conditions as chk
    fh, osc2, h = gk.project_rhs(mesh, k, f_ex)
    lv = galerkin_level(mesh, k, fh)
    u, G, ft, right, dir_f, cd = (lv[key] for key in ("u", "G", "ft", "right", "dirichlet", "cd"))
    s, wq = flux_rule(k)
    g = ALPHA * trace_values(mesh, k, right, u, s) if robin_flux else np.zeros((right.size, s.size))
    dofs = numpy_dofs(mesh, k, right.astype(np.int64), s, wq, g, False)[0]
    bv = dense_table(mesh, k, 1, {0: (right.astype(np.int64), dofs)})
    x = oracle_mod.se_reconstruct(mesh, k, ft, G[None], fh[None], boundary_values=bv)[0]
    res, nrm = chk.divergence_residual(mesh, k, x, G, fh)
    sig2 = flux_norm2_cells(mesh, k, x)
    osc = (h / np.pi) * np.sqrt(osc2)
    eta2 = float(np.sum((np.sqrt(sig2) + osc) ** 2))
    err2 = gk.energy_error(mesh, k, u, cd, grad_ex) ** 2 + boundary_error2(mesh, k, right, ALPHA, u)
    return dict(u=u, G=G, fh=fh, ft=ft, bv=bv, x=x, sig2=sig2, osc=osc, eta2=eta2, err2=err2, div_res=res / nrm,
                jump=chk.check_jump_condition(mesh, k, x, G, atol=1e-9), right=right, dirichlet=dir_f, h=h, osc2=osc2)
