"""The Robin term of the P_p Poisson operator on the host (dolfinx_eqlb_amd/lsolver/primal.py: set_robin): the table
FacetMass<p> in exact arithmetic and through the library's getter, the numpy statement against the Galerkin matrix
assembled by quadrature with the boundary mass (tests/robin_cases.py), the assembled matrix against apply, the solve
without a Dirichlet DOF, the refusals, and the host chain of the model problem of robin_cases.

The comparison of the statement is that of primal_cases.check_statement, entry by entry for apply and diagonal:
    |diff| <= 2^-53 (terms_s abs_s + terms_a abs_a)
with the chain counts of the plain operator plus, on the statement's side, ONE more rounding per Robin facet of a row
(at most FACETS_PER_ROW = 4, the pinched vertex of `bowtie`: each t_f[i] is one more addition to the value formed before;
the chain through a facet value itself - the weight 6, the contraction p + 1, one product - is shorter than the one it
joins) and on the assembled side one more addition, (A u) + (B u).  The abs-sums carry the new terms."""

from fractions import Fraction

import numpy as np
import pytest

import primal_cases as pc
import primal_mesh_cases as pm
import robin_cases as rb
from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
from dolfinx_eqlb_amd.lsolver import primal

U = pc.U
FACETS_PER_ROW = 4


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the table -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_facet_mass_table_against_fraction_integrals(p):
    M = primal.facet_mass_table_exact(p)
    n = p + 1
    assert len(M) == n and all(len(r) == n for r in M)
    assert all(isinstance(v, Fraction) for r in M for v in r)
    assert all(M[i][j] == M[j][i] for i in range(n) for j in range(n))
    assert sum(v for r in M for v in r) == 1
    # the basis is the nodal one of (0, 1, 1/p ... (p-1)/p), and the entries are its integrals: by an exact Gauss-free
    # route - the monomial moments int s^m = 1 / (m + 1) of the product of two interpolating polynomials
    nodes = [Fraction(0), Fraction(1)] + [Fraction(j, p) for j in range(1, p)]
    L = primal._lagrange_1d_exact(p)

    def value(c, x):
        return sum((a * x ** m for m, a in enumerate(c)), Fraction(0))
    for i in range(n):
        assert [value(L[i], x) for x in nodes] == [Fraction(int(i == k)) for k in range(n)]
        for j in range(n):
            prod = [Fraction(0)] * (2 * p + 1)
            for a, ca in enumerate(L[i]):
                for b, cb in enumerate(L[j]):
                    prod[a + b] += ca * cb
            assert M[i][j] == sum(c / (m + 1) for m, c in enumerate(prod))
    if p == 1:
        assert M == ((Fraction(1, 3), Fraction(1, 6)), (Fraction(1, 6), Fraction(1, 3)))
    assert np.array_equal(primal.facet_mass_table(p), np.array([[float(v) for v in r] for r in M]))


def test_getter_returns_the_doubles_of_the_generator():
    from dolfinx_eqlb_amd import cpp
    for p in range(1, 5):
        assert np.array_equal(bits(cpp.get_facet_mass_table(p)), bits(primal.facet_mass_table(p)))
    for bad in (0, 5):
        with pytest.raises(RuntimeError, match="eqlb_get_facet_mass_table: p = %d" % bad):
            cpp.get_facet_mass_table(bad)


# ---- the statement against the assembled stiffness + boundary mass ---------------------------------------------------
def case(name):
    """(mesh, Robin facets, alpha per facet, Dirichlet facets)"""
    if name == "square12":
        from dolfinx_eqlb_amd.mesh import create_unit_square
        mesh = create_unit_square(12, shuffle_seed=3, perturb=0.15)
        left, bottom, right, top = rb.sides(mesh)
        robin, dirichlet = np.concatenate([right, top]), left
    else:
        mesh = pm.mesh_of(name)
        robin, dirichlet = mesh.boundary_facets().astype(np.int32), np.zeros(0, dtype=np.int32)
    robin = robin[np.random.default_rng(5).permutation(robin.size)]          # (the list need not be sorted)
    return mesh, robin, rb.alpha_of(robin.size), dirichlet


def test_bowtie_has_a_row_in_four_robin_facets():
    mesh, robin, _, _ = case("bowtie")
    count = np.bincount(mesh.facet_nodes[robin].ravel(), minlength=mesh.nnodes)
    assert count.max() == FACETS_PER_ROW and (count == FACETS_PER_ROW).sum() == 1


@pytest.mark.parametrize("name", ["square12", "bowtie"])
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_statement_against_assembled_stiffness_and_boundary_mass(name, p):
    mesh, robin, alpha, dirichlet = case(name)
    assert (alpha == 0.0).sum() >= robin.size // 6 and alpha.max() > 5.0
    kappa = pc.kappa_of(mesh.ncells)
    op = primal.PoissonOperator(mesh, p, kappa)
    op.set_robin(robin, facet_alpha=alpha)
    A, Aabs = pc.assemble(mesh, p, kappa)[:2]
    B, Babs = rb.assemble_boundary_mass(mesh, p, robin, alpha)
    u = np.random.default_rng(9 + p).standard_normal(op.ndofs)
    ts, ta = pc.chain_terms(p, pm.valence(mesh), make_quadrature_triangle(2 * p + 4)[1].size)
    ts, ta = ts + FACETS_PER_ROW, ta + 1
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
    # the weights: alpha |E| with the square root of numpy, in the order of the list
    fn = mesh.facet_nodes[robin]
    dx, dy = mesh.x[fn[:, 1], 0] - mesh.x[fn[:, 0], 0], mesh.x[fn[:, 1], 1] - mesh.x[fn[:, 0], 1]
    assert np.array_equal(bits(op.robin_weights()), bits(alpha * np.sqrt(dx * dx + dy * dy)))
    # the load knows no Robin term; residual and mask go through apply
    d = min(p, 3)
    f = np.random.default_rng(p).standard_normal(mesh.ncells * (d + 1) * (d + 2) // 2)
    fresh = primal.PoissonOperator(mesh, p, kappa)
    assert np.array_equal(bits(op.load(d, f)), bits(fresh.load(d, f)))
    op.set_dirichlet(dirichlet if dirichlet.size else robin[:3])
    b = op.load(d, f)
    r = op.residual(b, u)
    assert np.array_equal(bits(r[~op.fixed]), bits((b - y)[~op.fixed])) and np.all(r[op.fixed] == 0.0)
    # an empty list: the operator of a fresh object, bit for bit
    op.set_robin([])
    assert np.array_equal(bits(op.apply(u)), bits(fresh.apply(u)))
    assert np.array_equal(bits(op.diagonal()), bits(fresh.diagonal()))
    assert op.robin_weights().size == 0


@pytest.mark.parametrize("name", ["square12", "bowtie"])
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_matrix_is_apply_column_by_column(name, p):
    """Bit for bit on every column that touches a Robin row (and a sample of the others): a column of the matrix has
    one term per row, so apply(e_j) forms the same sums with zeros in the other places - which change no bit but the
    sign of a zero"""
    mesh, robin, alpha, dirichlet = case(name)
    op = primal.PoissonOperator(mesh, p, pc.kappa_of(mesh.ncells))
    op.set_robin(robin, facet_alpha=alpha)
    op.set_dirichlet(dirichlet)
    ip, ix, v = op.matrix()
    n = op.ndofs
    import scipy.sparse as sp
    M = sp.csr_matrix((v, ix, ip), shape=(n, n)).tocsc()
    cols = np.unique(np.concatenate([primal.facet_dofs(mesh, p, robin).ravel(),
                                     np.random.default_rng(p).integers(0, n, 20)]))
    for j in cols:
        e = np.zeros(n)
        e[j] = 1.0
        y = op.apply(e)
        col = M.getcol(j).toarray().ravel()
        assert np.array_equal(bits(col + 0.0), bits(y + 0.0)), (name, p, j)
    assert np.array_equal(bits(M.diagonal()), bits(op.diagonal()))
    # eliminate acts as before
    ipe, ixe, ve = op.matrix(eliminate=True)
    rows = np.repeat(np.arange(n), np.diff(ip))
    fx = op.fixed[rows] | op.fixed[ix]
    assert np.array_equal(bits(ve), bits(np.where(fx, np.where(rows == ix, 1.0, 0.0), v)))


# ---- no Dirichlet DOF ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 3])
def test_all_robin_handle_converges_and_all_zero_alpha_is_refused(p):
    mesh = pm.mesh_of("bowtie")
    bf = mesh.boundary_facets()
    op = primal.PoissonOperator(mesh, p)
    op.set_robin(bf, alpha=2.0)
    assert not op.fixed.any() and op.robin_positive()
    b = np.random.default_rng(p).standard_normal(op.ndofs)
    u, info = op.pcg(b, np.zeros(op.ndofs), rtol=1e-10, maxit=4000)
    assert info["converged"] == 1 and info["breakdown"] == 0
    assert np.linalg.norm(b - op.apply(u)) <= 1e-9 * np.linalg.norm(b)
    op.set_robin(bf, alpha=0.0)
    assert not op.robin_positive()
    with pytest.raises(ValueError, match="singular: no Dirichlet DOF"):
        op.pcg(b, np.zeros(op.ndofs))
    op.set_robin([])
    with pytest.raises(ValueError, match="singular: no Dirichlet DOF"):
        op.pcg(b, np.zeros(op.ndofs))
    from dolfinx_eqlb_amd.lsolver import ElasticityOperator
    with pytest.raises(ValueError, match="PoissonOperator only"):
        ElasticityOperator(mesh, 1).set_robin(bf)


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_refusals_fire_by_name_and_leave_the_operator_as_it_was():
    mesh, robin, alpha, _ = case("square12")
    op = primal.PoissonOperator(mesh, 2)
    op.set_robin(robin, facet_alpha=alpha)
    u = np.random.default_rng(1).standard_normal(op.ndofs)
    y, d, w = op.apply(u), op.diagonal(), op.robin_weights()
    interior = int(np.nonzero(np.diff(mesh.facet_cells_offsets) == 2)[0][0])
    lst = robin.copy()
    lst[4] = interior
    with pytest.raises(ValueError, match=r"facets\[4\] = %d is no boundary facet" % interior):
        op.set_robin(lst, facet_alpha=alpha)
    for bad in (-1, mesh.nfacets):
        lst[4] = bad
        with pytest.raises(ValueError, match=r"facets\[4\] = %d is no boundary facet" % bad):
            op.set_robin(lst)
    lst = robin.copy()
    lst[7] = lst[2]
    with pytest.raises(ValueError, match=r"facets\[7\] = %d is listed twice" % lst[2]):
        op.set_robin(lst, facet_alpha=alpha)
    for value in (-1.0, np.nan, np.inf):
        a = alpha.copy()
        a[3] = value
        with pytest.raises(ValueError, match=r"facet_alpha\[3\]"):
            op.set_robin(robin, facet_alpha=a)
        with pytest.raises(ValueError, match="alpha = .* is negative, NaN or infinite"):
            op.set_robin(robin, alpha=value)
    with pytest.raises(ValueError, match="nlist"):
        op.set_robin(robin, facet_alpha=alpha[:-1])
    assert np.array_equal(bits(op.apply(u)), bits(y)) and np.array_equal(bits(op.diagonal()), bits(d))
    assert np.array_equal(bits(op.robin_weights()), bits(w))


# ---- robin_load, robin_flux, carry_robin_list --------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2, 4])
def test_robin_load_is_neumann_load_and_robin_flux_is_the_trace(p):
    from types import SimpleNamespace
    mesh, robin, alpha, _ = case("square12")

    def u_ext(x, y):
        return 1.0 + 0.5 * x - 0.25 * y * y
    b = primal.robin_load(mesh, p, robin, alpha, u_ext)
    bcs = [SimpleNamespace(facets=[int(f)], scalar=True, value=(lambda x, y, a=float(a): -a * u_ext(x, y)))
           for f, a in zip(robin, alpha)]
    assert np.array_equal(bits(b), bits(primal.neumann_load(mesh, p, bcs)))
    # int alpha u_ext phi_i: against the boundary mass applied to the interpolant of a u_ext in P_1
    lin = primal.robin_load(mesh, p, robin, alpha, lambda x, y: 1.0 + 0.5 * x - 0.25 * y)
    import galerkin as gk
    cd, ndofs = gk.dofmap(mesh, p)
    from dolfinx_eqlb_amd.elmtlib.lagrange import Lagrange
    from dolfinx_eqlb_amd.eqlb.check_eqlb_conditions import cell_geometry
    nodes = np.array([[float(a), float(c)] for a, c in Lagrange(p).nodes])
    xn = mesh.x[mesh.cell_nodes[:, 0], :2][:, None, :] + np.einsum("cij,qj->cqi", cell_geometry(mesh)[0], nodes)
    ui = np.zeros(ndofs)
    ui[cd.ravel()] = (1.0 + 0.5 * xn[..., 0] - 0.25 * xn[..., 1]).ravel()
    B = rb.assemble_boundary_mass(mesh, p, robin, alpha)[0]
    assert np.abs(lin - B @ ui).max() <= 1e-13 * np.abs(lin).max()
    # the flux condition: alpha (u_h - u_ext) at points of the facets, against the trace through the cell's basis
    u = np.random.default_rng(p).standard_normal(ndofs)
    s = np.array([0.0, 0.125, 0.5, 0.7, 1.0])
    ue = np.random.default_rng(p + 1).standard_normal((robin.size, s.size))
    got = primal.robin_flux(mesh, p, robin, alpha, u, s, ue)
    ref = alpha[:, None] * (rb.trace_values(mesh, p, robin, u, s) - ue)
    assert np.abs(got - ref).max() <= 1e-13 * max(np.abs(ref).max(), 1.0)
    assert np.array_equal(primal.robin_flux(mesh, p, robin, alpha, u, s),
                          primal.robin_flux(mesh, p, robin, alpha, u, s, np.zeros_like(ue)))


def test_carry_robin_list_follows_child_facets():
    from dolfinx_eqlb_amd.mesh import refine
    mesh, robin, alpha, _ = case("square12")
    marked = np.arange(0, mesh.ncells, 3)
    x2, cells2, _, npf = refine.refine_longest_edge(mesh, marked)
    from dolfinx_eqlb_amd.mesh import create_mesh
    mesh2 = create_mesh(x2[:, :2], cells2)
    f2, a2 = refine.carry_robin_list(mesh, npf, mesh2, robin, alpha)
    assert f2.size > robin.size and np.all(np.diff(mesh2.facet_cells_offsets)[f2] == 1) and np.unique(f2).size == f2.size
    pf = refine.parent_facets(mesh, npf, mesh2)
    lookup = dict(zip(robin.tolist(), alpha.tolist()))
    assert all(lookup[int(pf[f])] == a for f, a in zip(f2, a2))
    assert np.isclose(np.sum(a2 * primal.facet_lengths(mesh2, f2)), np.sum(alpha * primal.facet_lengths(mesh, robin)))
    primal.PoissonOperator(mesh2, 2).set_robin(f2, facet_alpha=a2)


# ---- the host chain --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3])
def test_host_chain_bounds_the_error_with_the_flux_condition_of_the_solution(oracle_mod, k):
    """Galerkin solve with the boundary mass -> sigma_h = -grad u_h -> the oracle with boundary_values = the moments of
    alpha u_h on the Robin side -> eta.  With sigma_eq . n = alpha (u_h - u_ext) there the boundary residual drops out
    of the Prager-Synge argument and eta bounds the error in |||e|||^2 = || grad e ||^2 + || alpha^(1/2) e ||^2 on the
    Robin side.  The flux space RT_k carries the facet moments 0 ... k - 1 of alpha u_h, whose trace has degree k: at
    flux degree k = primal degree the top moment of alpha u_h is dropped.  The omitted boundary oscillation is of higher
    order and is NOT part of the guarantee asserted here - the bound holds with the margins printed below.  With a zero
    flux prescribed on the Robin side instead, eta / e exceeds 10: the reason the flux kernel exists."""
    for n in (4, 8):
        mesh = rb.chain_mesh(n)
        lv = rb.host_level(oracle_mod, mesh, k)
        eff = np.sqrt(lv["eta2"] / lv["err2"])
        print(f"k={k} n={n}: eta / e = {eff:.3f}, relative divergence residual {lv['div_res']:.2e}")
        assert lv["eta2"] >= lv["err2"]
        assert lv["div_res"] < 1e-9 and lv["jump"]
        zero = rb.host_level(oracle_mod, mesh, k, robin_flux=False)
        ratio = np.sqrt(zero["eta2"] / zero["err2"])
        print(f"k={k} n={n}: with a zero flux on the Robin side eta / e = {ratio:.1f}")
        if n == 8:
            assert ratio > 10.0
