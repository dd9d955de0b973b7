"""The reaction term of the P_p solves and the value projection, on the host: the two new tables in exact arithmetic
and through the library's getters, and the numpy statement (dolfinx_eqlb_amd/lsolver/primal.py: set_reaction) against an
independently rounded assembly - the quadrature mass matrix of tests/reaction_cases.py beside primal_cases.assemble /
elasticity_cases.assemble.

The comparison is that of primal_cases.check_statement, entry by entry for apply and diagonal:
    |diff| <= 2^-53 (terms_s abs_s + terms_a abs_a)
with the chain counts of the plain operator and ONE more rounding on either side (reaction_cases.chain_terms counts
them): the statement adds wm m[i] to the value it formed before, the assembled side adds M u to A u; the chains through
the new terms themselves are shorter than the ones they join.  The abs-sums carry the new terms (return_abs; |M|)."""

from fractions import Fraction

import numpy as np
import pytest

import elasticity_cases as ec
import primal_cases as pc
import reaction_cases as rc
from dolfinx_eqlb_amd.elmtlib.lagrange import Lagrange
from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
from dolfinx_eqlb_amd.lsolver import primal

U = rc.U


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the tables, in Fractions ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_mass_table_is_symmetric_and_sums_to_the_area(p):
    M = primal.mass_table_exact(p)
    n = len(M)
    assert n == (p + 1) * (p + 2) // 2 and all(len(r) == n for r in M)
    assert all(isinstance(v, Fraction) for r in M for v in r)
    assert all(M[i][j] == M[j][i] for i in range(n) for j in range(n))
    assert sum(v for r in M for v in r) == Fraction(1, 2)
    assert np.array_equal(primal.mass_table(p), np.array([[float(v) for v in r] for r in M]))


@pytest.mark.parametrize("p", [1, 2, 3])
def test_load_table_of_equal_degrees_is_the_mass_table(p):
    assert primal.load_table_exact(p, p) == primal.mass_table_exact(p)


def _value(poly, x, y):
    return sum((c * x ** a * y ** b for (a, b), c in poly.items()), Fraction(0))


@pytest.mark.parametrize("p", [1, 2, 3, 4])
@pytest.mark.parametrize("d", [0, 1, 2, 3])
def test_value_table_reproduces_monomials_and_is_the_projection(p, d):
    PV = primal.value_table_exact(p, d)
    el, dg = Lagrange(p), Lagrange(d)
    assert len(PV) == dg.ndofs and all(len(r) == el.ndofs for r in PV)
    for deg in range(min(p, d) + 1):
        for a in range(deg + 1):
            mono = {(a, deg - a): Fraction(1)}
            u = [_value(mono, *node) for node in el.nodes]          # the monomial lies in P_p: its nodal values
            got = [sum(PV[n][i] * u[i] for i in range(el.ndofs)) for n in range(dg.ndofs)]
            assert got == [_value(mono, *node) for node in dg.nodes], (p, d, a, deg - a)
    if d < p:
        Md, L = primal.mass_table_exact(d), primal.load_table_exact(p, d)
        for n in range(dg.ndofs):
            for i in range(el.ndofs):
                assert sum(Md[n][m] * PV[m][i] for m in range(dg.ndofs)) == L[i][n], (p, d, n, i)


def test_getters_return_the_doubles_of_the_generator():
    from dolfinx_eqlb_amd import cpp
    for p in range(1, 5):
        assert np.array_equal(bits(cpp.get_mass_table(p)), bits(primal.mass_table(p)))
        for d in range(4):
            assert np.array_equal(bits(cpp.get_value_table(p, d)), bits(primal.value_table(p, d)))
    for bad in (0, 5):
        with pytest.raises(RuntimeError, match="eqlb_get_mass_table: p = %d" % bad):
            cpp.get_mass_table(bad)
    with pytest.raises(RuntimeError, match="eqlb_get_value_table"):
        cpp.get_value_table(1, 4)


# ---- the statement against the assembled stiffness + mass -----------------------------------------------------------
def make_op(problem, mesh, p):
    if problem == "poisson":
        coeff = pc.kappa_of(mesh.ncells)
        return primal.PoissonOperator(mesh, p, coeff), coeff, pc.assemble(mesh, p, coeff)[:2]
    coeff = ec.pi1_of(mesh.ncells)
    return primal.ElasticityOperator(mesh, p, cell_pi1=coeff), coeff, ec.assemble(mesh, p, 1.0, coeff)[:2]


@pytest.mark.parametrize("problem", ["poisson", "elasticity"])
@pytest.mark.parametrize("name", rc.STATEMENT_MESHES)
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_statement_against_assembled_stiffness_and_mass(problem, name, p):
    mesh = rc.mesh_of(name)
    bs = 1 if problem == "poisson" else 2
    c = rc.c_of(mesh.ncells)
    assert (c == 0.0).sum() >= mesh.ncells // 7 and c.max() > 1e3 and c[c > 0].min() < 1e-1
    op, _, (A, Aabs) = make_op(problem, mesh, p)
    op.set_reaction(cell_c=c)
    M, Mabs = rc.assemble_mass(mesh, p, c, bs)
    u = np.random.default_rng(9 + p).standard_normal(bs * op.ndofs)
    valence = int(np.diff(mesh.node_cells_offsets).max())
    ts, ta = rc.chain_terms(problem, p, valence, make_quadrature_triangle(2 * p + 4)[1].size)
    y, yabs = op.apply(u, return_abs=True)
    diff = np.abs(y - (A @ u + M @ u))
    bound = U * (ts * yabs + ta * (Aabs @ np.abs(u) + Mabs @ np.abs(u)))
    r_apply = pc.ratio(diff, bound)
    assert np.any(np.abs(y - A @ u) > bound)     # the term is there: without it the difference leaves the bound
    dg, dabs = op.diagonal(return_abs=True)
    ddiff = np.abs(dg - (A.diagonal() + M.diagonal()))
    dbound = U * (ts * dabs + ta * (Aabs.diagonal() + Mabs.diagonal()))
    r_diag = pc.ratio(ddiff, dbound)
    print(f"{problem} {name} p={p}: largest |diff| / bound: apply {r_apply:.3f}, diagonal {r_diag:.3f} (terms {(ts, ta)})")
    assert np.all(diff <= bound)
    assert np.all(ddiff <= dbound) and np.all(dg > 0.0)
    # the load knows no reaction term; residual and mask go through apply
    d = min(p, 3)
    f = np.random.default_rng(p).standard_normal((bs, mesh.ncells * (d + 1) * (d + 2) // 2))
    fresh = make_op(problem, mesh, p)[0]
    assert np.array_equal(bits(op.load(d, f)), bits(fresh.load(d, f)))
    bf = mesh.boundary_facets()
    op.set_dirichlet(*([bf] * bs))
    b = op.load(d, f)
    r = op.residual(b, u)
    assert np.array_equal(bits(r[~op.fixed]), bits((b - y)[~op.fixed])) and np.all(r[op.fixed] == 0.0)


@pytest.mark.parametrize("problem", ["poisson", "elasticity"])
@pytest.mark.parametrize("p", [1, 3])
def test_scalar_is_the_constant_array_and_zero_is_a_fresh_operator(problem, p):
    mesh = rc.mesh_of("base9")
    bs = 1 if problem == "poisson" else 2
    op, fresh = make_op(problem, mesh, p)[0], make_op(problem, mesh, p)[0]
    u = np.random.default_rng(p).standard_normal(bs * op.ndofs)
    y0, d0 = fresh.apply(u), fresh.diagonal()
    op.set_reaction(2.5)
    ys, ds = op.apply(u), op.diagonal()
    assert not np.array_equal(ys, y0) and np.all(ds > d0)
    op.set_reaction(cell_c=np.full(mesh.ncells, 2.5))
    assert np.array_equal(bits(op.apply(u)), bits(ys)) and np.array_equal(bits(op.diagonal()), bits(ds))
    op.set_reaction(0.0)
    assert np.array_equal(bits(op.apply(u)), bits(y0)) and np.array_equal(bits(op.diagonal()), bits(d0))
    ya, aa = op.apply(u, return_abs=True)
    yb, ab = fresh.apply(u, return_abs=True)
    assert np.array_equal(bits(ya), bits(yb)) and np.array_equal(bits(aa), bits(ab))
    # an array of zeros keeps the term (one product and one addition of +0) and changes no value
    op.set_reaction(cell_c=np.zeros(mesh.ncells))
    assert np.array_equal(op.apply(u), y0) and np.array_equal(op.diagonal(), d0)
    # refusals name the cell and leave the operator as it was
    op.set_reaction(1.5)
    y1 = op.apply(u)
    bad = np.ones(mesh.ncells)
    for value, where in ((-1.0, 5), (np.nan, 0), (np.inf, mesh.ncells - 1)):
        cc = bad.copy()
        cc[where] = value
        with pytest.raises(ValueError, match=r"cell_c\[%d\]" % where):
            op.set_reaction(cell_c=cc)
    with pytest.raises(ValueError, match="negative"):
        op.set_reaction(-2.0)
    with pytest.raises(ValueError, match="ncells"):
        op.set_reaction(cell_c=np.ones(mesh.ncells + 1))
    assert np.array_equal(bits(op.apply(u)), bits(y1))


@pytest.mark.parametrize("p,d", [(1, 0), (2, 1), (3, 3), (4, 2)])
def test_value_statement_is_the_l2_projection(p, d):
    """value_dg against the L2 projection by quadrature of the same function: M_d x = int psi_n u_h per cell, to the
    accuracy of a dense solve of a well-conditioned nd_d x nd_d system"""
    from dolfinx_eqlb_amd.mesh.transfer import lagrange_dofmap
    mesh = rc.mesh_of("base9")
    cd, ndofs = lagrange_dofmap(mesh, p)
    u = np.random.default_rng(p + d).standard_normal(ndofs)
    c = rc.c_of(mesh.ncells)
    qp, qw = make_quadrature_triangle(p + d + 2)
    phi, psi = Lagrange(p).tabulate(qp)[0], Lagrange(d).tabulate(qp)[0]
    Md = np.einsum("q,qn,qm->nm", qw, psi, psi)
    rhs = np.einsum("q,qn,qi,ci->cn", qw, psi, phi, u[cd])
    ref = c[:, None] * np.linalg.solve(Md, rhs.T).T
    got, A = primal.value_dg(p, d, cd, u, c, return_abs=True)
    nd = (d + 1) * (d + 2) // 2
    assert got.shape == (1, mesh.ncells * nd)
    assert np.abs(got[0] - ref.ravel()).max() <= 1e-11 * max(np.abs(ref).max(), 1.0)
    assert np.all(np.abs(got) <= A * (1 + 64 * U))
    plain = primal.value_dg(p, d, cd, np.stack([u, 2 * u]))
    assert plain.shape == (2, mesh.ncells * nd) and np.array_equal(bits(plain[1]), bits(2 * plain[0]))
    tab = primal.value_table(p, d)
    assert np.array_equal(bits(primal.value_dg(p, d, cd, u, c, op=tab)), bits(got))
