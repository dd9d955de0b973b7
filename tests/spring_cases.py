"""Shared by tests/test_primal_springs_host.py and the tests/test_gpu_*springs*.py files: the spring lists and tensors of
the cases, the boundary term int_E phi_i^T K phi_j assembled by quadrature (the independently rounded computation the
spring term of dolfinx_eqlb_amd/lsolver/primal.py is compared with), and the model problem of the chains.  No test lives
here.

The tensors: facet-wise random, every fifth exactly zero, every third (of the rest) rank one from spring_tensor(kn, 0),
the others full with eigenvalues in [0.5, 10] and a correlation up to 0.8 of either sign.

THE MODEL PROBLEM.  The unit square with u = 0 on x = 0, y = 0, y = 1 and a spring side x = 1 with K = 10 n x n + 1 t x t
(n = e_x there, so K = diag(10, 1)); pi_1 = 1.  Manufactured u = sin(pi y) (x, x (1 + x)), f = -div sigma(u) by sympy,
u_ext = u + K^-1 sigma(u) n on the spring side, so that sigma(u) n = -K (u - u_ext) holds.  The error is measured in
|||e|||^2 = int 2 eps(e) : eps(e) + pi_1 (div e)^2 + int_Gamma e^T K e."""

import numpy as np
import scipy.sparse as sp

import elasticity_cases as ec
import galerkin as gk
import primal_mesh_cases as pm
import robin_cases as rb
from dolfinx_eqlb_amd.lsolver import primal

U = ec.U
FACETS_PER_ROW = 4          # the pinched vertex of `bowtie`
KN, KT, PI_1 = 10.0, 1.0, 1.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def tensors_of(mesh, facets, seed=17):
    """facet_k [n, 3] in the order of `facets`: every fifth zero, every third rank one (normal stiffness), the rest full"""
    facets = np.asarray(facets, dtype=np.int64)
    rng = np.random.default_rng(seed)
    n = facets.size
    a, b = 0.5 + 9.5 * rng.random(n), 0.5 + 9.5 * rng.random(n)
    c = 1.6 * rng.random(n) - 0.8
    K = np.stack([a, c * np.sqrt(a * b), b], axis=1)
    i = np.arange(n)
    one = (i % 3 == 0)
    K[one] = primal.spring_tensor(mesh, facets[one], 10.0 * rng.random(int(one.sum())) + 0.1, 0.0)
    K[i % 5 == 0] = 0.0
    return K


def kinds(K):
    """(zero, rank one, definite) counts of a tensor array"""
    zero = ~np.any(K, axis=1)
    definite = primal.spring_definite(K)
    return int(zero.sum()), int((~zero & ~definite).sum()), int(definite.sum())


def layout(name):
    """(mesh, spring facets in a shuffled order, facet_k, the two Dirichlet lists)"""
    none = np.zeros(0, dtype=np.int32)
    if name == "square576":
        from dolfinx_eqlb_amd.mesh import create_unit_square
        mesh = create_unit_square(12, shuffle_seed=3, perturb=0.15)
        assert mesh.ncells == 576
        left, bottom, right, top = rb.sides(mesh)
        springs, fixed = np.concatenate([right, top]), (left, left)
    else:
        mesh = pm.mesh_of(name)
        springs = (pm.dirichlet_facets(mesh, "inner") if name == "hole" else mesh.boundary_facets()).astype(np.int32)
        fixed = (none, none)
    springs = springs[np.random.default_rng(5).permutation(springs.size)].astype(np.int32)
    return mesh, springs, tensors_of(mesh, springs), tuple(np.asarray(f, dtype=np.int32) for f in fixed)


def assemble_boundary_springs(mesh, p, facets, K):
    """(B csr [2 ndofs, 2 ndofs], |B|) blocked: entry (2 i + r, 2 j + s) = sum_f K_f[r][s] int_E phi_i phi_j, every
    component pair through robin_cases.assemble_boundary_mass - Gauss quadrature of degree 2 p + 2 from the basis of the
    facet's cell, which knows nothing of the local order of a facet's rows"""
    ndofs = gk.dofmap(mesh, p)[1]
    B = sp.csr_matrix((2 * ndofs, 2 * ndofs))
    Babs = sp.csr_matrix((2 * ndofs, 2 * ndofs))
    for r in range(2):
        for s in range(2):
            M = rb.assemble_boundary_mass(mesh, p, facets, K[:, r + s])[0].tocoo()
            Ma = rb.assemble_boundary_mass(mesh, p, facets, np.abs(K[:, r + s]))[1].tocoo()
            B = B + sp.csr_matrix((M.data, (2 * M.row + r, 2 * M.col + s)), shape=B.shape)
            Babs = Babs + sp.csr_matrix((Ma.data, (2 * Ma.row + r, 2 * Ma.col + s)), shape=B.shape)
    return B.tocsr(), Babs.tocsr()


# ---- the model problem -------------------------------------------------------------------------------------------------
_EXACT = {}


def exact():
    """dict(u [2], gu [2][2] (gu[r][d] = d_d u_r), f [2], u_ext [2]): callables (x, y) -> arrays"""
    if not _EXACT:
        import sympy as sy
        x, y = sy.symbols("x y")
        u = [sy.sin(sy.pi * y) * x, sy.sin(sy.pi * y) * x * (1 + x)]
        gu = [[sy.diff(u[r], v) for v in (x, y)] for r in range(2)]
        div = gu[0][0] + gu[1][1]
        pi = sy.nsimplify(PI_1)
        sig = [[gu[r][d] + gu[d][r] + (pi * div if r == d else 0) for d in range(2)] for r in range(2)]
        f = [-(sy.diff(sig[r][0], x) + sy.diff(sig[r][1], y)) for r in range(2)]
        # on x = 1: n = e_x, K = diag(KN, KT); sigma n = -K (u - u_ext)  =>  u_ext = u + K^-1 sigma n
        ue = [u[0] + sig[0][0] / sy.nsimplify(KN), u[1] + sig[1][0] / sy.nsimplify(KT)]

        def fn(e):
            g = sy.lambdify((x, y), e, "numpy")
            return lambda a, b: g(a, b) + 0.0 * a
        _EXACT.update(u=[fn(e) for e in u], gu=[[fn(e) for e in row] for row in gu], f=[fn(e) for e in f],
                      u_ext=[fn(e) for e in ue])
    return _EXACT


def chain_mesh(n):
    return rb.chain_mesh(n)


def chain_layout(mesh):
    """(spring facets = the side x = 1, facet_k, the Dirichlet facets (both rows), ft [2, nfacets])"""
    left, bottom, right, top = rb.sides(mesh)
    K = primal.spring_tensor(mesh, right, KN, KT)
    assert np.abs(K - np.array([KN, 0.0, KT])).max() < 1e-12
    fixed = np.concatenate([left, bottom, top]).astype(np.int32)
    ft = np.zeros((2, mesh.nfacets), dtype=np.int8)
    ft[:, mesh.boundary_facets()] = 1
    ft[:, right] = 2
    return right, K, fixed, ft


def u_ext_points(mesh, facets, s):
    """u_ext [2, n, nq] at the facet parameters s of the listed facets (the frame of eqlb_facet_points)"""
    from dolfinx_eqlb_amd.eqlb.bcs import _facet_points
    from dolfinx_eqlb_amd.eqlb.check_eqlb_conditions import cell_geometry
    cells, lf = rb.facet_geometry(mesh, facets)
    pts = _facet_points(np.asarray(s, dtype=np.float64))
    xq = mesh.x[mesh.cell_nodes[cells, 0], :2][:, None, :] + np.einsum("cij,cqj->cqi", cell_geometry(mesh)[0][cells],
                                                                        pts[lf])
    ex = exact()
    return np.stack([ex["u_ext"][r](xq[..., 0], xq[..., 1]) for r in range(2)]), xq


def trace_values(mesh, p, facets, u, s):
    """u_h [2, n, nq] from the basis of the facet's cell (robin_cases.trace_values per component)"""
    uu = np.asarray(u, dtype=np.float64).reshape(-1, 2)
    return np.stack([rb.trace_values(mesh, p, facets, np.ascontiguousarray(uu[:, r]), s) for r in range(2)])


def boundary_error2(mesh, p, facets, K, u):
    """int_Gamma e^T K e over the listed facets (Gauss rule of degree 2 p + 6)"""
    from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_interval
    s, wq = make_quadrature_interval(2 * p + 6)
    _, xq = u_ext_points(mesh, facets, s)
    ex = exact()
    e = np.stack([ex["u"][r](xq[..., 0], xq[..., 1]) for r in range(2)]) - trace_values(mesh, p, facets, u, s)
    E = primal.facet_lengths(mesh, facets)
    dens = K[:, 0, None] * e[0] ** 2 + 2.0 * K[:, 1, None] * e[0] * e[1] + K[:, 2, None] * e[1] ** 2
    return float(np.sum(E[:, None] * wq[None, :] * dens))


def bulk_error2(mesh, k, u, cd):
    """int 2 eps(e) : eps(e) + pi_1 (div e)^2 by quadrature of degree 2 k + 6"""
    from dolfinx_eqlb_amd.elmtlib.lagrange import Lagrange
    from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
    from dolfinx_eqlb_amd.eqlb.check_eqlb_conditions import cell_geometry
    import shear_cases as sc
    J, detJ, Kc = cell_geometry(mesh)
    qp, qw = make_quadrature_triangle(2 * k + 6)
    tab = Lagrange(k).tabulate(qp, 1)
    dphi = np.stack([tab[1], tab[2]], axis=2)
    guh = np.einsum("cXd,qiX,cir->cqrd", Kc, dphi, np.asarray(u).reshape(-1, 2)[cd])
    xq, yq = sc.points(mesh, qp)
    ex = exact()
    ge = np.stack([np.stack([ex["gu"][r][d](xq, yq) for d in range(2)], axis=-1) for r in range(2)], axis=-2) - guh
    eps = 0.5 * (ge + np.swapaxes(ge, 2, 3))
    dens = 2.0 * np.einsum("cqrd,cqrd->cq", eps, eps) + PI_1 * (ge[..., 0, 0] + ge[..., 1, 1]) ** 2
    return float(np.sum(qw[None, :] * np.abs(detJ)[:, None] * dens))


def problem(n, k):
    """The P_k Galerkin solution of the model problem on chain_mesh(n) (sparse direct solve of the matrix assembled by
    quadrature with the boundary term) and what the equilibration and the estimate need."""
    import scipy.sparse.linalg as spla
    import shear_cases as sc
    from dolfinx_eqlb_amd.elmtlib.lagrange import Lagrange
    from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
    from dolfinx_eqlb_amd.eqlb.check_eqlb_conditions import cell_geometry
    ex = exact()
    mesh = chain_mesh(n)
    springs, K, fixed_f, ft = chain_layout(mesh)
    A = ec.assemble(mesh, k, PI_1)[0] + assemble_boundary_springs(mesh, k, springs, K)[0]
    cd, ndofs = gk.dofmap(mesh, k)
    detJ = cell_geometry(mesh)[1]
    qp, qw = make_quadrature_triangle(2 * k + 6)
    tab = Lagrange(k).tabulate(qp, 1)
    w = qw[None, :] * np.abs(detJ)[:, None]
    xq, yq = sc.points(mesh, qp)
    b = np.zeros(2 * ndofs)
    for r in range(2):
        np.add.at(b, (2 * cd + r).ravel(), np.einsum("cq,cq,qi->ci", w, ex["f"][r](xq, yq), tab[0]).ravel())
    b_spring = primal.spring_load(mesh, k, springs, K, lambda x, y: (ex["u_ext"][0](x, y), ex["u_ext"][1](x, y)))
    b = b + b_spring
    fixed = np.repeat(primal.dirichlet_mask(mesh, k, fixed_f), 2)
    free = np.nonzero(~fixed)[0]
    u = np.zeros(2 * ndofs)
    u[free] = spla.spsolve(A.tocsr()[free][:, free].tocsc(), b[free])
    fh, osc2 = [], 0.0
    for r in range(2):
        fr, o2, h = gk.project_rhs(mesh, k, ex["f"][r])
        fh.append(fr)
        osc2 = osc2 + o2
    pi = np.full(mesh.ncells, PI_1)
    G = sc.stress_rows(mesh, k, u.reshape(ndofs, 2), cd, pi, np.ones(mesh.ncells))
    err2 = bulk_error2(mesh, k, u, cd) + boundary_error2(mesh, k, springs, K, u)
    return dict(mesh=mesh, springs=springs, K=K, fixed_f=fixed_f, ft=ft, cd=cd, b=b, b_spring=b_spring, u=u, fixed=fixed,
                G=G, fh=np.stack(fh), osc2=osc2, h=h, err=float(np.sqrt(err2)))


def flux_table(mesh, k, springs, g, s, wq):
    """boundary_values of the oracle from the point values g [2, n, nq] of the two flux conditions on `springs`"""
    from test_gpu_bc_update import dense_table, numpy_dofs
    f64 = np.asarray(springs, dtype=np.int64)
    return dense_table(mesh, k, 2, {r: (f64, numpy_dofs(mesh, k, f64, s, wq, g[r], False)[0]) for r in range(2)})


def host_terms(oracle_mod, P, k, spring_flux=True):
    """(energy, wsym, osc per cell, relative divergence residual) of the host chain: the oracle with weak symmetry and
    Korn constants and boundary_values = the moments of K (u_h - u_ext) on the spring side (spring_flux=False: a zero
    traction prescribed there), stress_estimator_terms, the oscillation with the Korn constants"""
    from dolfinx_eqlb_amd.eqlb import check_eqlb_conditions as chk
    mesh, springs = P["mesh"], P["springs"]
    s, wq = rb.flux_rule(k)
    if spring_flux:
        ue, _ = u_ext_points(mesh, springs, s)
        g = primal.spring_flux(mesh, k, springs, P["K"], P["u"], s, ue)
    else:
        g = np.zeros((2, springs.size, s.size))
    bv = flux_table(mesh, k, springs, g, s, wq)
    x = oracle_mod.se_reconstruct(mesh, k, P["ft"], P["G"], P["fh"], stress=True, boundary_values=bv)
    rel = 0.0
    for r in range(2):
        res, nrm = chk.divergence_residual(mesh, k, x[r], P["G"][r], P["fh"][r])
        rel = max(rel, res / nrm)
    korn = np.sqrt(oracle_mod.se_korn(mesh, P["ft"]))
    energy, wsym = chk.stress_estimator_terms(mesh, k, x, korn, cell_pi1=np.full(mesh.ncells, PI_1))
    return energy, wsym, korn ** 2 * (P["h"] / np.pi) ** 2 * P["osc2"], rel
