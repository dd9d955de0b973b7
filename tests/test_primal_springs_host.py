"""The spring term of the P_p^2 elasticity operator on the host (dolfinx_eqlb_amd/lsolver/primal.py: set_springs): the
numpy statement against the Galerkin matrix assembled by quadrature with the boundary term int_E phi_i^T K phi_j
(tests/spring_cases.py), the assembled matrix against apply, the refusals by name, the allowance of the semidefiniteness
test, the solve without a Dirichlet DOF, spring_load / spring_flux / carry_springs_list, and the host chain of the model
problem of spring_cases.

The comparison of the statement is that of primal_cases.check_statement, entry by entry for apply and diagonal:
    |diff| <= 2^-53 (terms_s abs_s + terms_a abs_a)
with the chain counts of the plain elasticity operator (elasticity_cases.chain_terms) plus
  statement   ONE more rounding per spring facet of a row, at most FACETS_PER_ROW = 4 (the pinched vertex of `bowtie`):
              each t_f[i][r] is one more addition to the value formed before.  The chain through a facet value itself
              is shorter than the one it joins: the length |E| 6 (two differences, two squares, a sum, a root), its
              product with k 1, the contraction p + 1, the two products with Kw and their sum 2 - p + 10 <= 14 against
              the 28 + nd_p >= 31 of a cell value in front of the owner sum
  assembled   one more addition, (A u) + (B u).  The chain of (B u) - tabulation 2 (p + 3), the length 6, the Gauss
              rule of p + 2 points with its products p + 6, the product with k 1, the sum over at most 4 facets 4, the
              product with u over both components of the p + 1 rows of at most 4 facets 8 (p + 1) - stays below the
              one of (A u) on every mesh here but the one- and two-cell meshes at p >= 3, where it is longer by at
              most 8: 8 is added on the assembled side throughout.
The abs-sums carry the new terms, with |K| entry by entry (k01 has either sign)."""

import numpy as np
import pytest

import elasticity_cases as ec
import primal_cases as pc
import primal_mesh_cases as pm
import robin_cases as rb
import spring_cases as sp_
from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
from dolfinx_eqlb_amd.lsolver import primal
from spring_cases import bits

U = pc.U
NAMES = ("bowtie", "triangle", "right1", "hole", "two_parts", "square576")


def operator(name, p, springs=True):
    mesh, facets, K, fixed = sp_.layout(name)
    op = primal.ElasticityOperator(mesh, p, cell_pi1=ec.pi1_of(mesh.ncells))
    if springs:
        op.set_springs(facets, facet_k=K)
    return op, mesh, facets, K, fixed


def test_the_tensors_cover_zero_rank_one_and_full():
    for name in NAMES:
        mesh, facets, K, _ = sp_.layout(name)
        zero, one, full = sp_.kinds(K)
        assert zero >= 1 and zero + one + full == facets.size
        if facets.size >= 8:
            assert one >= 1 and full >= 2, (name, zero, one, full)
        primal.spring_list("test", mesh, facets, facet_k=K)
    mesh, facets, _, _ = sp_.layout("bowtie")
    count = np.bincount(mesh.facet_nodes[facets].ravel(), minlength=mesh.nnodes)
    assert count.max() == sp_.FACETS_PER_ROW


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_statement_against_assembled_stiffness_and_boundary_term(name, p):
    op, mesh, facets, K, fixed = operator(name, p)
    cell_pi1 = ec.pi1_of(mesh.ncells)
    A, Aabs = ec.assemble(mesh, p, 1.0, cell_pi1)[:2]
    B, Babs = sp_.assemble_boundary_springs(mesh, p, facets, K)
    u = np.random.default_rng(9 + p).standard_normal(2 * op.ndofs)
    ts, ta = ec.chain_terms(p, pm.valence(mesh), make_quadrature_triangle(2 * p + 4)[1].size)
    ts, ta = ts + sp_.FACETS_PER_ROW, ta + 1 + 8
    y, yabs = op.apply(u, return_abs=True)
    diff = np.abs(y - (A @ u + B @ u))
    bound = U * (ts * yabs + ta * (Aabs @ np.abs(u) + Babs @ np.abs(u)))
    assert np.any(np.abs(y - A @ u) > bound)     # the term is there: without it the difference leaves the bound
    dg, dabs = op.diagonal(return_abs=True)
    ddiff = np.abs(dg - (A.diagonal() + B.diagonal()))
    dbound = U * (ts * dabs + ta * (Aabs.diagonal() + Babs.diagonal()))
    print(f"{name} p={p}: largest |diff| / bound: apply {pc.ratio(diff, bound):.3f}, diagonal "
          f"{pc.ratio(ddiff, dbound):.3f} (terms {(ts, ta)})")
    assert np.all(diff <= bound)
    assert np.all(ddiff <= dbound) and np.all(dg > 0.0)
    # the weights: |E| k entry by entry with the square root of numpy, in the order of the list
    fn = mesh.facet_nodes[facets]
    dx, dy = mesh.x[fn[:, 1], 0] - mesh.x[fn[:, 0], 0], mesh.x[fn[:, 1], 1] - mesh.x[fn[:, 0], 1]
    assert np.array_equal(bits(op.spring_weights()), bits(np.sqrt(dx * dx + dy * dy)[:, None] * K))
    # the load knows no spring term; residual and mask go through apply
    d = min(p, 3)
    f = np.random.default_rng(p).standard_normal((2, mesh.ncells * (d + 1) * (d + 2) // 2))
    fresh = primal.ElasticityOperator(mesh, p, cell_pi1=cell_pi1)
    assert np.array_equal(bits(op.load(d, f)), bits(fresh.load(d, f)))
    op.set_dirichlet(facets[:3], facets[1:2])
    b = op.load(d, f)
    r = op.residual(b, u)
    assert np.array_equal(bits(r[~op.fixed]), bits((b - y)[~op.fixed])) and np.all(r[op.fixed] == 0.0)
    # an empty list: the operator of a fresh object, bit for bit
    op.set_springs([])
    assert np.array_equal(bits(op.apply(u)), bits(fresh.apply(u)))
    assert np.array_equal(bits(op.diagonal()), bits(fresh.diagonal()))
    assert op.spring_weights().shape == (0, 3) and not op.spring_positive()


@pytest.mark.parametrize("name", ["square576", "bowtie", "triangle"])
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_matrix_is_apply_column_by_column(name, p):
    """Bit for bit on every column that touches a spring row (and a sample of the others), as for the Robin term; the
    raw diagonal has the bits of diagonal(), eliminate acts as before"""
    import scipy.sparse as sps
    op, mesh, facets, K, fixed = operator(name, p)
    op.set_dirichlet(fixed[0], facets[:2])
    ip, ix, v = op.matrix()
    n = 2 * op.ndofs
    M = sps.csr_matrix((v, ix, ip), shape=(n, n)).tocsc()
    fd = primal.facet_dofs(mesh, p, facets).ravel()
    cols = np.unique(np.concatenate([2 * fd, 2 * fd + 1, np.random.default_rng(p).integers(0, n, 20)]))
    for j in cols:
        e = np.zeros(n)
        e[j] = 1.0
        assert np.array_equal(bits(M.getcol(j).toarray().ravel() + 0.0), bits(op.apply(e) + 0.0)), (name, p, j)
    assert np.array_equal(bits(M.diagonal()), bits(op.diagonal()))
    ipe, ixe, ve = op.matrix(eliminate=True)
    rows = np.repeat(np.arange(n), np.diff(ip))
    fx = op.fixed[rows] | op.fixed[ix]
    assert np.array_equal(bits(ve), bits(np.where(fx, np.where(rows == ix, 1.0, 0.0), v)))
    fresh = operator(name, p, springs=False)[0]
    assert np.array_equal(ip, fresh.matrix()[0]) and np.array_equal(ix, fresh.matrix()[1])     # no pattern changes


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_refusals_fire_by_name_and_leave_the_operator_as_it_was():
    op, mesh, facets, K, _ = operator("square576", 2)
    u = np.random.default_rng(1).standard_normal(2 * op.ndofs)
    y, d, w = op.apply(u), op.diagonal(), op.spring_weights()
    interior = int(np.nonzero(np.diff(mesh.facet_cells_offsets) == 2)[0][0])
    for bad in (interior, -1, mesh.nfacets):
        lst = facets.copy()
        lst[4] = bad
        with pytest.raises(ValueError, match=r"facets\[4\] = %d is no boundary facet" % bad):
            op.set_springs(lst, facet_k=K)
    lst = facets.copy()
    lst[7] = lst[2]
    with pytest.raises(ValueError, match=r"facets\[7\] = %d is listed twice" % lst[2]):
        op.set_springs(lst, facet_k=K)
    for col in range(3):
        for value in (np.nan, np.inf, -np.inf):
            k = K.copy()
            k[3, col] = value
            with pytest.raises(ValueError, match=r"facet_k\[3\] = .* is not finite"):
                op.set_springs(facets, facet_k=k)
    k = K.copy()
    k[3] = (-1.0, 0.0, 2.0)
    with pytest.raises(ValueError, match=r"facet_k\[3\]: k00 = -1.0 is negative"):
        op.set_springs(facets, facet_k=k)
    k[3] = (2.0, 0.0, -0.5)
    with pytest.raises(ValueError, match=r"facet_k\[3\]: k11 = -0.5 is negative"):
        op.set_springs(facets, facet_k=k)
    k[3] = (1.0, 1.0 + 1e-14, 1.0)
    with pytest.raises(ValueError, match=r"facet_k\[3\] = .* is not positive semidefinite"):
        op.set_springs(facets, facet_k=k)
    # the order of the tests: the facet before its tensor, an earlier facet before a later one
    k[2] = (np.nan, 0.0, 1.0)
    with pytest.raises(ValueError, match=r"facet_k\[2\] = .* is not finite"):
        op.set_springs(facets, facet_k=k)
    lst = facets.copy()
    lst[1] = interior
    with pytest.raises(ValueError, match=r"facets\[1\] = %d is no boundary facet" % interior):
        op.set_springs(lst, facet_k=k)
    for value in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="k = .* is negative, NaN or infinite"):
            op.set_springs(facets, k=value)
    with pytest.raises(ValueError, match="nlist"):
        op.set_springs(facets, facet_k=K[:-1])
    with pytest.raises(ValueError, match="PoissonOperator only"):
        op.set_robin(facets)
    assert np.array_equal(bits(op.apply(u)), bits(y)) and np.array_equal(bits(op.diagonal()), bits(d))
    assert np.array_equal(bits(op.spring_weights()), bits(w))
    # the scalar form is k I; a tensor on the edge of the allowance passes
    op.set_springs(facets, k=2.5)
    ref = primal.ElasticityOperator(mesh, 2, cell_pi1=ec.pi1_of(mesh.ncells))
    ref.set_springs(facets, facet_k=np.tile([2.5, 0.0, 2.5], (facets.size, 1)))
    assert np.array_equal(bits(op.apply(u)), bits(ref.apply(u)))
    k = K.copy()
    k[3] = (1.0, 1.0 + 2.0 ** -52, 1.0)
    op.set_springs(facets, facet_k=k)


def test_spring_tensor_passes_the_allowance_on_a_million_normals():
    """kn n_a n_b in floating point: k01 k01 and k00 k11 differ by a few roundings, which the allowance 2^-49 = 16
    units of 2^-53 covers; with kt > 0 the tensor is definite by a margin far above it.  The largest excess is printed."""
    rng = np.random.default_rng(0)
    m = 10 ** 6
    th = rng.uniform(0.0, 2.0 * np.pi, m)
    n = np.stack([np.cos(th), np.sin(th)], axis=1)
    n[:4] = [[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [np.sqrt(0.5), np.sqrt(0.5)]]
    kn, kt = 10.0 ** rng.uniform(-6.0, 6.0, m), 10.0 ** rng.uniform(-6.0, 6.0, m)
    kt[::3] = 0.0
    K = primal.spring_tensor_of_normals(n, kn, kt)
    assert np.all(np.isfinite(K)) and np.all(K[:, 0] >= 0.0) and np.all(K[:, 2] >= 0.0)
    assert np.all(primal.spring_semidefinite(K))
    prod = K[:, 0] * K[:, 2]
    excess = np.where(prod > 0.0, K[:, 1] * K[:, 1] / np.where(prod > 0.0, prod, 1.0) - 1.0, 0.0)[kt == 0.0]
    print(f"rank one: largest k01^2 / (k00 k11) - 1 = {excess.max() / U:.1f} units of 2^-53 (allowance 16)")
    assert excess.max() <= primal.SPRING_ALLOWANCE
    assert not np.any(primal.spring_definite(K)[kt == 0.0]) and np.all(primal.spring_definite(K)[kt > 0.0])
    # spring_list is the same test, facet by facet: on the boundary of a mesh
    mesh = pm.mesh_of("hole")
    bf = mesh.boundary_facets()
    for kt_ in (0.0, 1e-6, 3.0):
        Kf = primal.spring_tensor(mesh, bf, 1e6, kt_)
        primal.spring_list("test", mesh, bf, facet_k=Kf)
        nrm = primal.facet_normals(mesh, bf)
        assert np.allclose(np.sum(nrm * nrm, axis=1), 1.0)
        assert np.allclose(Kf[:, 0] + Kf[:, 2], 1e6 + kt_)          # the trace
    # the normals point outwards: away from the middle on the outer loop, towards it on the inner one
    inner = np.isin(bf, pm.dirichlet_facets(mesh, "inner"))
    d = mesh.facet_midpoints()[bf][:, :2] - 0.5
    out = np.sum(primal.facet_normals(mesh, bf) * d, axis=1)
    assert np.all(out[~inner] > 0.0) and np.all(out[inner] < 0.0)


# ---- no Dirichlet DOF ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 3])
def test_full_rank_springs_need_no_dirichlet_dof_and_rank_one_springs_do(p):
    import scipy.sparse as sps
    import scipy.sparse.linalg as spla
    from dolfinx_eqlb_amd.mesh import create_unit_square
    mesh = create_unit_square(6, shuffle_seed=3, perturb=0.15)
    bf = mesh.boundary_facets()
    op = primal.ElasticityOperator(mesh, p, 2.0)
    op.set_springs(bf, facet_k=primal.spring_tensor(mesh, bf, 5.0, 0.5))
    assert not op.fixed.any() and op.spring_positive()
    n = 2 * op.ndofs
    b = np.random.default_rng(p).standard_normal(n)
    u, info = op.pcg(b, np.zeros(n), rtol=1e-11, maxit=20000)
    assert info["converged"] == 1 and info["breakdown"] == 0
    ip, ix, v = op.matrix()
    ref = spla.spsolve(sps.csr_matrix((v, ix, ip), shape=(n, n)).tocsc(), b)
    assert np.abs(u - ref).max() <= 1e-8 * np.abs(ref).max()
    # rank one only: the per-component rule stays in force
    op.set_springs(bf, facet_k=primal.spring_tensor(mesh, bf, 5.0, 0.0))
    assert not op.spring_positive()
    with pytest.raises(ValueError, match="singular: component 0 has no Dirichlet DOF"):
        op.pcg(b, np.zeros(n))
    left = rb.sides(mesh)[0]
    op.set_dirichlet(left, [])
    with pytest.raises(ValueError, match="singular: component 1 has no Dirichlet DOF"):
        op.pcg(b, np.zeros(n))
    op.set_springs([])
    with pytest.raises(ValueError, match="singular: component 1 has no Dirichlet DOF"):
        op.pcg(b, np.zeros(n))


@pytest.mark.parametrize("p", [1, 2])
def test_hierarchy_carries_the_term_and_its_coarse_solve_needs_no_dirichlet_dof(p):
    from dolfinx_eqlb_amd.lsolver import Hierarchy
    from dolfinx_eqlb_amd.mesh import refine
    meshes, links = pm.levels_host("sq6_two")
    ops, f, K = [], None, None
    for l, m in enumerate(meshes):
        op = primal.ElasticityOperator(m, p, 2.0)
        if l == 0:
            f = m.boundary_facets().astype(np.int32)
            K = sp_.tensors_of(m, f)
        else:
            f, K = refine.carry_springs_list(meshes[l - 1], links[l - 1][1], m, f, K)
        op.set_springs(f, facet_k=K)
        ops.append(op)
    assert ops[0].spring_positive() and not ops[0].fixed.any()

    class Link:
        def __init__(self, link):
            self.parent_cell, self.node_parent_facet = link
    refs = [Link(x) for x in links]
    n = ops[-1].fixed.size
    b = np.random.default_rng(p).standard_normal(n)
    for local, coarse in ((False, False), (True, True)):
        H = Hierarchy(ops, refs, local=local, coarse=coarse)
        u, info = H.pcg(b, np.zeros(n), rtol=1e-10, maxit=2000)
        assert info["converged"] == 1 and info["breakdown"] == 0
        r = ops[-1].residual(b, u)
        assert np.sqrt(np.sum(r * r)) <= 1.01e-10 * ops[-1].reference_norm(b, np.zeros(n))
    for op in ops:
        op.set_springs(op.mesh.boundary_facets(), facet_k=primal.spring_tensor(op.mesh, op.mesh.boundary_facets(), 1.0))
    with pytest.raises(ValueError, match="no Dirichlet DOF"):
        Hierarchy(ops, refs, coarse=True)


# ---- spring_load, spring_flux, carry_springs_list ------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2, 4])
def test_spring_load_is_traction_load_and_spring_flux_is_the_trace(p):
    from types import SimpleNamespace
    mesh, facets, K, _ = sp_.layout("square576")

    def u_ext(x, y):
        return 1.0 + 0.5 * x - 0.25 * y, -0.5 + x * y
    b = primal.spring_load(mesh, p, facets, K, u_ext)
    rows = [[SimpleNamespace(facets=[int(f)], scalar=True,
                             value=(lambda x, y, a=float(k[r]), c=float(k[r + 1]):
                                    -(a * np.asarray(u_ext(x, y)[0]) + c * np.asarray(u_ext(x, y)[1]))))
             for f, k in zip(facets, K)] for r in range(2)]
    assert np.array_equal(bits(b), bits(primal.traction_load(mesh, p, rows)))
    # int phi_i (K u_ext)_r against the boundary term applied to the interpolant of a u_ext in P_1
    lin = primal.spring_load(mesh, p, facets, K, lambda x, y: (1.0 + 0.5 * x - 0.25 * y, -0.5 + x - y))
    import galerkin as gk
    from dolfinx_eqlb_amd.elmtlib.lagrange import Lagrange
    from dolfinx_eqlb_amd.eqlb.check_eqlb_conditions import cell_geometry
    cd, ndofs = gk.dofmap(mesh, p)
    nodes = np.array([[float(a), float(c)] for a, c in Lagrange(p).nodes])
    xn = mesh.x[mesh.cell_nodes[:, 0], :2][:, None, :] + np.einsum("cij,qj->cqi", cell_geometry(mesh)[0], nodes)
    ui = np.zeros((ndofs, 2))
    ui[cd.ravel(), 0] = (1.0 + 0.5 * xn[..., 0] - 0.25 * xn[..., 1]).ravel()
    ui[cd.ravel(), 1] = (-0.5 + xn[..., 0] - xn[..., 1]).ravel()
    B = sp_.assemble_boundary_springs(mesh, p, facets, K)[0]
    assert np.abs(lin - B @ ui.ravel()).max() <= 1e-13 * np.abs(lin).max()
    # the flux conditions: K (u_h - u_ext) at points of the facets, against the trace through the cell's basis
    u = np.random.default_rng(p).standard_normal(2 * ndofs)
    s = np.array([0.0, 0.125, 0.5, 0.7, 1.0])
    ue = np.random.default_rng(p + 1).standard_normal((2, facets.size, s.size))
    got = primal.spring_flux(mesh, p, facets, K, u, s, ue)
    d = sp_.trace_values(mesh, p, facets, u, s) - ue
    ref = np.stack([K[:, r, None] * d[0] + K[:, r + 1, None] * d[1] for r in range(2)])
    assert got.shape == (2, facets.size, s.size)
    assert np.abs(got - ref).max() <= 1e-13 * max(np.abs(ref).max(), 1.0)
    assert np.array_equal(primal.spring_flux(mesh, p, facets, K, u, s),
                          primal.spring_flux(mesh, p, facets, K, u, s, np.zeros_like(ue)))


def test_carry_springs_list_follows_child_facets():
    from dolfinx_eqlb_amd.mesh import create_mesh, refine
    mesh, facets, K, _ = sp_.layout("square576")
    x2, cells2, _, npf = refine.refine_longest_edge(mesh, np.arange(0, mesh.ncells, 3))
    mesh2 = create_mesh(x2[:, :2], cells2)
    f2, K2 = refine.carry_springs_list(mesh, npf, mesh2, facets, K)
    assert f2.size > facets.size and K2.shape == (f2.size, 3) and np.unique(f2).size == f2.size
    assert np.all(np.diff(mesh2.facet_cells_offsets)[f2] == 1)
    pf = refine.parent_facets(mesh, npf, mesh2)
    lookup = {int(f): k for f, k in zip(facets, K)}
    assert all(np.array_equal(bits(lookup[int(pf[f])]), bits(k)) for f, k in zip(f2, K2))
    # the same list as the Robin rule, component by component
    for c in range(3):
        fr, ar = refine.carry_robin_list(mesh, npf, mesh2, facets, K[:, c])
        assert np.array_equal(fr, f2) and np.array_equal(bits(ar), bits(K2[:, c]))
    primal.ElasticityOperator(mesh2, 2).set_springs(f2, facet_k=K2)


# ---- the host chain --------------------------------------------------------------------------------------------------
# eta / e of the host chain, measured (printed by the test below).  The estimator carries no term for
# the part of K (u_h - u_ext) beyond degree k - 1 on a facet, so the bound is asserted exactly on the cases of HOLDS.
HOLDS = {(2, 4), (2, 8), (2, 16), (3, 4), (3, 8), (3, 16)}


@pytest.mark.parametrize("k", [2, 3])
def test_host_chain_of_the_model_problem(oracle_mod, k):
    """Galerkin solve with the boundary term -> sigma_h -> the oracle with weak symmetry, Korn constants and
    boundary_values = the moments of K (u_h - u_ext) on the spring side for both stress rows -> eta, against the error
    in |||e|||^2 = bulk energy + int_Gamma e^T K e.  With a zero traction prescribed on the spring side instead eta / e
    is far from one: the condition matters."""
    import shear_cases as sc
    for n in (4, 8, 16):
        P = sp_.problem(n, k)
        energy, wsym, osc, rel = sp_.host_terms(oracle_mod, P, k)
        eff = sc.estimate(energy, wsym, osc) / P["err"]
        zero = sp_.host_terms(oracle_mod, P, k, spring_flux=False)
        ratio = sc.estimate(*zero[:3]) / P["err"]
        print(f"k={k} n={n}: e = {P['err']:.4e}, eta / e = {eff:.4f}, relative divergence residual {rel:.2e}; with a "
              f"zero traction on the spring side eta / e = {ratio:.2f}")
        assert rel < 1e-9
        if (k, n) in HOLDS:
            assert eff >= 1.0 - 1e-10
        if n >= 8:
            assert ratio > 2.0 * eff
