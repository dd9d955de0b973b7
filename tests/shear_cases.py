"""Shared by tests/test_primal_shear_host.py and tests/test_gpu_shear_chain.py: the Galerkin matrix of
-div(mu (2 eps(u) + pi_1 div(u) I)) with mu_T inside the integral, put together from elasticity_cases.assemble per
distinct value of mu on the cells that carry it, and the bimaterial square with its exact solution and its host chain.
No test lives here.

THE BIMATERIAL SQUARE.  Interface x = 1/2; mu = 1 and pi_1 = 1 on the left, mu = mu2 and pi_1 = 2 on the right.  The mesh
is the perturbed crossed unit square of the other estimator tests with the nodes of the grid line x = 1/2 put back onto
it, so no cell straddles the interface.  Exact solution, with w = x (1 - x) y (1 - y) (1, 1 + x):
    u_0 = (x - 1/2) w_0 / (mu (2 + pi_1)),   u_1 = (x - 1/2) w_1 / mu      (mu, pi_1 of the side).
It vanishes on the boundary and on the interface.  On x = 1/2 only d_x u is left, d_x u_0 = w_0 / (mu (2 + pi_1)) and
d_x u_1 = w_1 / mu, so the traction sigma e_x = mu ((2 + pi_1) d_x u_0, d_x u_1) = (w_0, w_1) is the same from both sides:
-div(sigma) = f holds with f taken per side (sympy) and no interface load.
(u = (x - 1/2) w / mu in both components - continuous mu grad(u) - has a continuous traction only where pi_1 does not
jump: its normal traction is (2 + pi_1) w_0, a jump of w_0 between pi_1 = 1 and 2.  The P_k solutions then converge to
another function and the error against it stalls at 1.1e-2 from n = 8 on; hence the factor 1 / (2 + pi_1) in u_0.)"""

import numpy as np

import elasticity_cases as ec
import galerkin as gk
from dolfinx_eqlb_amd.eqlb import check_eqlb_conditions as chk

PI_LEFT, PI_RIGHT = 1.0, 2.0


# ---- mu inside the integral ----------------------------------------------------------------------------------------------
def restricted(mesh, p, sel, cell_pi1):
    """(A, |A|) of elasticity_cases.assemble on the cells `sel` alone, in the numbering of the whole mesh: assembled on
    the mesh of those cells (same nodes, same local vertex order) and moved by the map of its DOFs - a vertex keeps its
    id, a facet is found by its node pair, a cell by its place in sel."""
    import scipy.sparse as sp
    from dolfinx_eqlb_amd.mesh import create_mesh
    sel = np.asarray(sel, dtype=np.int64)
    sub = create_mesh(mesh.x[:, :2], mesh.cell_nodes[sel])
    A, Aabs = ec.assemble(sub, p, 1.0, np.asarray(cell_pi1)[sel])[:2]
    nn, ne, ni = mesh.nnodes, p - 1, (p - 1) * (p - 2) // 2
    key = lambda m: m.facet_nodes[:, 0].astype(np.int64) * nn + m.facet_nodes[:, 1]   # noqa: E731 (sorted: create_mesh)
    full_keys = key(mesh)
    facet = np.searchsorted(full_keys, key(sub))
    assert np.array_equal(full_keys[facet], key(sub))
    ndofs_sub = nn + sub.nfacets * ne + sub.ncells * ni
    ndofs = nn + mesh.nfacets * ne + mesh.ncells * ni
    to = np.empty(ndofs_sub, dtype=np.int64)
    to[:nn] = np.arange(nn)
    to[nn:nn + sub.nfacets * ne] = (nn + facet[:, None] * ne + np.arange(ne)[None, :]).ravel()
    to[nn + sub.nfacets * ne:] = (nn + mesh.nfacets * ne + sel[:, None] * ni + np.arange(ni)[None, :]).ravel()
    to2 = (2 * to[:, None] + np.arange(2)[None, :]).ravel()
    P = sp.csr_matrix((np.ones(to2.size), (to2, np.arange(to2.size))), shape=(2 * ndofs, 2 * ndofs_sub))
    return (P @ A @ P.T).tocsr(), (P @ Aabs @ P.T).tocsr()


def assemble_mu(mesh, p, cell_pi1, cell_mu):
    """(A, |A|, number of distinct values): sum over the distinct values v of cell_mu of v * restricted(cells with v)"""
    mu = np.asarray(cell_mu, dtype=np.float64)
    A = Aabs = None
    values = np.unique(mu)
    for v in values:
        Av, Aa = restricted(mesh, p, np.nonzero(mu == v)[0], cell_pi1)
        A = v * Av if A is None else A + v * Av
        Aabs = v * Aa if Aabs is None else Aabs + v * Aa
    return A.tocsr(), Aabs.tocsr(), values.size


# ---- the bimaterial square ------------------------------------------------------------------------------------------------
_EXACT = {}


def bimaterial_mesh(n):
    from dolfinx_eqlb_amd.mesh import create_mesh, create_unit_square
    assert n % 2 == 0
    m = create_unit_square(n, shuffle_seed=3, perturb=0.15)
    x = m.x[:, :2].copy()
    grid = np.arange((n + 1) * (n + 1))                    # the corner nodes come first, row by row
    on = grid[grid % (n + 1) == n // 2]
    assert np.all(np.abs(x[on, 0] - 0.5) < 0.15 / n)
    x[on, 0] = 0.5
    mesh = create_mesh(x, m.cell_nodes)
    xc = mesh.x[mesh.cell_nodes, 0]
    right = xc.mean(axis=1) > 0.5
    assert np.all(xc[right] >= 0.5) and np.all(xc[~right] <= 0.5) and right.sum() == mesh.ncells // 2
    return mesh, right


def exact(mu2):
    """(u [2], grad u [2][2] (gu[r][d] = d_d u_r), f [2]): callables (x, y) -> arrays, per side by the sign of x - 1/2"""
    if mu2 not in _EXACT:
        import sympy as sy
        x, y = sy.symbols("x y")
        w = [x * (1 - x) * y * (1 - y), x * (1 - x) * y * (1 - y) * (1 + x)]
        sides = []
        for mu, pi in ((1, PI_LEFT), (mu2, PI_RIGHT)):
            u = [(x - sy.Rational(1, 2)) * w[0] / (mu * (2 + sy.nsimplify(pi))), (x - sy.Rational(1, 2)) * w[1] / mu]
            gu = [[sy.diff(u[r], v) for v in (x, y)] for r in range(2)]
            div = gu[0][0] + gu[1][1]
            sig = [[mu * (gu[r][d] + gu[d][r] + (pi * div if r == d else 0)) for d in range(2)] for r in range(2)]
            f = [-(sy.diff(sig[r][0], x) + sy.diff(sig[r][1], y)) for r in range(2)]
            sides.append((u, gu, f))

        def fn(left, right):
            gl, gr = sy.lambdify((x, y), left, "numpy"), sy.lambdify((x, y), right, "numpy")
            return lambda a, b: np.where(a < 0.5, gl(a, b) + 0.0 * a, gr(a, b) + 0.0 * a)
        (ul, gl, fl), (ur, gr, fr) = sides
        _EXACT[mu2] = dict(u=[fn(ul[r], ur[r]) for r in range(2)],
                           gu=[[fn(gl[r][d], gr[r][d]) for d in range(2)] for r in range(2)],
                           f=[fn(fl[r], fr[r]) for r in range(2)])
    return _EXACT[mu2]


def points(mesh, qp):
    """the images of the reference points: x, y [ncells, nq]"""
    J = chk.cell_geometry(mesh)[0]
    xq = mesh.x[mesh.cell_nodes[:, 0], :2][:, None, :] + np.einsum("cij,qj->cqi", J, qp)
    return xq[..., 0], xq[..., 1]


def side_fn(mesh, right, g):
    """g(x, y) evaluated with the side taken from the cell, not from x: for arrays [ncells, nq]"""
    def f(a, b):
        xs = np.where(right[:, None], np.maximum(a, 0.5), np.minimum(a, np.nextafter(0.5, 0.0)))
        return g(xs, b)
    return f


def energy_error(mesh, k, u, cd, ex, cell_pi1, cell_mu, right):
    """sqrt(int mu (2 eps(e) : eps(e) + pi_1 (div e)^2)), e = u - u_h, by quadrature of degree 2 k + 6"""
    from dolfinx_eqlb_amd.elmtlib.lagrange import Lagrange
    from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
    J, detJ, K = chk.cell_geometry(mesh)
    qp, qw = make_quadrature_triangle(2 * k + 6)
    tab = Lagrange(k).tabulate(qp, 1)
    dphi = np.stack([tab[1], tab[2]], axis=2)
    guh = np.einsum("cXd,qiX,cir->cqrd", K, dphi, u[cd])
    xq, yq = points(mesh, qp)
    ge = np.stack([np.stack([side_fn(mesh, right, ex["gu"][r][d])(xq, yq) for d in range(2)], axis=-1)
                   for r in range(2)], axis=-2) - guh
    eps = 0.5 * (ge + np.swapaxes(ge, 2, 3))
    dens = 2.0 * np.einsum("cqrd,cqrd->cq", eps, eps) + cell_pi1[:, None] * (ge[..., 0, 0] + ge[..., 1, 1]) ** 2
    return float(np.sqrt(np.sum(qw[None, :] * (np.abs(detJ) * cell_mu)[:, None] * dens)))


def stress_rows(mesh, k, u, cd, cell_pi1, cell_mu):
    """rows of -mu (2 eps(u_h) + pi_1 div(u_h) I) at the DG_{k-1} nodes: [2, ncells*nd*2]"""
    from test_estimator_bound import elasticity_stress_rows
    G = elasticity_stress_rows(mesh, k, u, cd, np.asarray(cell_pi1)[:, None])
    return np.ascontiguousarray((G.reshape(2, mesh.ncells, -1) * np.asarray(cell_mu)[None, :, None]).reshape(2, -1))


def problem(n, k, mu2):
    """The P_k Galerkin solution (sparse direct solve of the matrix with mu inside the integral) on bimaterial_mesh(n)
    and what the equilibration and the estimate need, as test_estimator_bound.elasticity_problem returns it, with
    cell_pi1, cell_mu and right."""
    import scipy.sparse.linalg as spla
    from dolfinx_eqlb_amd.elmtlib.lagrange import Lagrange
    from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
    from synthetic import facet_types
    ex = exact(mu2)
    mesh, right = bimaterial_mesh(n)
    cell_pi1 = np.where(right, PI_RIGHT, PI_LEFT)
    cell_mu = np.where(right, float(mu2), 1.0)
    A = assemble_mu(mesh, k, cell_pi1, cell_mu)[0]
    cd, ndofs = gk.dofmap(mesh, k)
    J, detJ, K = chk.cell_geometry(mesh)
    qp, qw = make_quadrature_triangle(2 * k + 6)
    tab = Lagrange(k).tabulate(qp, 1)
    w = qw[None, :] * np.abs(detJ)[:, None]
    xq, yq = points(mesh, qp)
    f = [side_fn(mesh, right, ex["f"][r]) for r in range(2)]
    b = np.zeros(2 * ndofs)
    for r in range(2):
        np.add.at(b, (2 * cd + r).ravel(), np.einsum("cq,cq,qi->ci", w, f[r](xq, yq), tab[0]).ravel())
    bf = mesh.boundary_facets()
    fixed = np.zeros(ndofs, dtype=bool)
    fixed[mesh.facet_nodes[bf].ravel()] = True
    for j in range(k - 1):
        fixed[mesh.nnodes + bf * (k - 1) + j] = True
    free = np.nonzero(~np.repeat(fixed, 2))[0]
    u = np.zeros(2 * ndofs)
    u[free] = spla.spsolve(A[free][:, free].tocsc(), b[free])
    u = u.reshape(ndofs, 2)
    fh, osc2 = [], 0.0
    for r in range(2):
        fr, o2, h = gk.project_rhs(mesh, k, f[r])
        fh.append(fr)
        osc2 = osc2 + o2
    ft = np.repeat(facet_types(mesh, None), 2, axis=0)
    return dict(mesh=mesh, right=right, cell_pi1=cell_pi1, cell_mu=cell_mu, ft=ft, cd=cd, b=b, u=u, f=f, fixed=fixed,
                G=stress_rows(mesh, k, u, cd, cell_pi1, cell_mu), fh=np.stack(fh), osc2=osc2, h=h,
                err=energy_error(mesh, k, u, cd, ex, cell_pi1, cell_mu, right))


def host_terms(oracle_mod, P, k):
    """(energy, wsym, osc per cell, C_K per cell) of the host chain: the oracle with weak symmetry and Korn constants,
    stress_estimator_terms with cell_pi1 and cell_mu, the oscillation with korn / sqrt(mu)"""
    mesh = P["mesh"]
    x = oracle_mod.se_reconstruct(mesh, k, P["ft"], P["G"], P["fh"], stress=True)
    for r in range(2):
        res, nrm = chk.divergence_residual(mesh, k, x[r], P["G"][r], P["fh"][r])
        assert res < 1e-9 * nrm
    korn = np.sqrt(oracle_mod.se_korn(mesh, P["ft"]))
    energy, wsym = chk.stress_estimator_terms(mesh, k, x, korn, cell_pi1=P["cell_pi1"], cell_mu=P["cell_mu"])
    kw = korn / np.sqrt(P["cell_mu"])
    return energy, wsym, kw ** 2 * (P["h"] / np.pi) ** 2 * P["osc2"], korn


def estimate(energy, wsym, osc):
    """eta as the reference's estimate() sums it with guarantied_upper_bound=True"""
    return float(np.sqrt(np.sum(energy) + np.sum((np.sqrt(wsym) + np.sqrt(osc)) ** 2)))
