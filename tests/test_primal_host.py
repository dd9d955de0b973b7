"""The P_p Poisson solve as far as it can be checked without a device: the tables Stiff<p> and Load<p,d> against
quadrature and bit for bit against the library, the numpy statement (dolfinx_eqlb_amd/lsolver/primal.py) against the
assembled Galerkin matrix, its PCG against a direct solve, neumann_load, and the refusals of the ABI that come before
the device is touched."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import primal_cases as pc
from dolfinx_eqlb_amd.elmtlib.lagrange import Lagrange
from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
from dolfinx_eqlb_amd.lsolver import primal
from dolfinx_eqlb_amd.mesh import create_mesh, create_unit_square, refine_longest_edge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = -1
U = pc.U
ENTRIES = ("eqlb_get_stiffness_table", "eqlb_get_load_table", "eqlb_primal_create", "eqlb_primal_ndofs",
           "eqlb_primal_set_dirichlet", "eqlb_primal_load", "eqlb_primal_apply", "eqlb_primal_diagonal",
           "eqlb_primal_residual", "eqlb_primal_solve")


def _meshes():
    sq = create_unit_square(3, shuffle_seed=1)
    import refine_cases
    ls, marked = refine_cases.case("lshape")
    x2, c2, _, _ = refine_longest_edge(ls, marked)
    return {"sq3": sq, "lshape_refined": create_mesh(x2[:, :2], c2)}


MESHES = _meshes()


_ratio = pc.ratio


# ---- tables ---------------------------------------------------------------------------------------------------------
def _abs_tab(el, pts, nderiv):
    """tabulate with the absolute value of every monomial term: the abs-sum of the evaluation"""
    from dolfinx_eqlb_amd.elmtlib import polynomials as P
    out = np.zeros((3, pts.shape[0], el.ndofs))
    for i, b in enumerate(el.basis):
        for n, poly in enumerate((b, P.ddx(b), P.ddy(b))):
            out[n, :, i] = P.evaluate({k: abs(v) for k, v in poly.items()}, pts)
    return out


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_stiffness_table_equals_quadrature(p):
    """|table - quadrature| <= terms 2^-53 abs-sum: abs-sum = sum_q w_q sum |monomials of d phi_i| sum |monomials of
    d phi_j|; terms = the roundings of one chain: nq sums, two polynomial evaluations of at most nd_p monomials with
    powers up to p (nd_p + p + 1 each), 3 products, the rounding of points and weights (4) and of the table entry (1)."""
    el = Lagrange(p)
    qp, qw = make_quadrature_triangle(2 * p)
    t, a = el.tabulate(qp, 1), _abs_tab(el, qp, 1)
    S = primal.stiffness_table(p)
    terms = qw.size + 2 * (el.ndofs + p + 1) + 3 + 4 + 1
    quad = [np.einsum("q,qi,qj->ij", qw, t[1], t[1]),
            np.einsum("q,qi,qj->ij", qw, t[1], t[2]) + np.einsum("q,qi,qj->ij", qw, t[2], t[1]),
            np.einsum("q,qi,qj->ij", qw, t[2], t[2])]
    asum = [np.einsum("q,qi,qj->ij", qw, a[1], a[1]),
            np.einsum("q,qi,qj->ij", qw, a[1], a[2]) + np.einsum("q,qi,qj->ij", qw, a[2], a[1]),
            np.einsum("q,qi,qj->ij", qw, a[2], a[2])]
    for m in range(3):
        diff, bound = np.abs(S[m] - quad[m]), terms * U * asum[m]
        print(f"Stiff<{p}> S{m}: max |diff| / bound = {_ratio(diff, bound):.3f}")
        assert np.all(diff <= bound)
        assert np.array_equal(S[m], S[m].T)
    # constants lie in the kernel
    assert np.abs(S.sum(axis=2)).max() <= 3 * el.ndofs * U * np.abs(S).sum(axis=2).max()


@pytest.mark.parametrize("p", [1, 2, 3, 4])
@pytest.mark.parametrize("d", [0, 1, 2, 3])
def test_load_table_equals_quadrature(p, d):
    el, dg = Lagrange(p), Lagrange(d)
    qp, qw = make_quadrature_triangle(p + d)
    t, a = el.tabulate(qp)[0], _abs_tab(el, qp, 0)[0]
    s, b = dg.tabulate(qp)[0], _abs_tab(dg, qp, 0)[0]
    L = primal.load_table(p, d)
    terms = qw.size + (el.ndofs + p + 1) + (dg.ndofs + d + 1) + 3 + 4 + 1
    diff, bound = np.abs(L - np.einsum("q,qi,qn->in", qw, t, s)), terms * U * np.einsum("q,qi,qn->in", qw, a, b)
    print(f"Load<{p},{d}>: max |diff| / bound = {_ratio(diff, bound):.3f}")
    assert np.all(diff <= bound)
    # sum_n chi_n = 1: the rows sum to int phi_i
    assert abs(L.sum() - 0.5) <= L.size * U


def test_library_tables_are_the_generated_ones():
    from dolfinx_eqlb_amd import cpp
    for p in range(1, 5):
        assert np.array_equal(cpp.get_stiffness_table(p), primal.stiffness_table(p))
        for d in range(4):
            assert np.array_equal(cpp.get_load_table(p, d), primal.load_table(p, d))
    L = cpp.lib()
    buf = np.zeros(4)
    for p in (0, 5):
        assert L.eqlb_get_stiffness_table(C.c_int32(p), buf.ctypes.data_as(C.c_void_p), C.c_int32(4)) == INVALID_ARGUMENT
        assert L.eqlb_get_load_table(C.c_int32(p), C.c_int32(0), buf.ctypes.data_as(C.c_void_p), C.c_int32(4)) \
            == INVALID_ARGUMENT
    for d in (-1, 4):
        assert L.eqlb_get_load_table(C.c_int32(1), C.c_int32(d), buf.ctypes.data_as(C.c_void_p), C.c_int32(4)) \
            == INVALID_ARGUMENT
    assert L.eqlb_get_stiffness_table(C.c_int32(2), buf.ctypes.data_as(C.c_void_p), C.c_int32(4)) == INVALID_ARGUMENT
    assert "capacity" in L.eqlb_last_error().decode()


# ---- the statement against the assembled matrix --------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MESHES))
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_statement_equals_the_assembled_operator(name, p):
    pc.check_statement(MESHES[name], p, name)


def test_dirichlet_mask_replaces_and_refuses():
    mesh = MESHES["sq3"]
    op = primal.PoissonOperator(mesh, 3)
    bf = mesh.boundary_facets()
    op.set_dirichlet(bf)
    op.set_dirichlet(bf[:1])
    assert op.fixed.sum() == 2 + 2
    with pytest.raises(ValueError, match="no facet"):
        op.set_dirichlet([mesh.nfacets])
    with pytest.raises(ValueError, match="no Dirichlet"):
        primal.PoissonOperator(mesh, 1).pcg(np.zeros(mesh.nnodes), np.zeros(mesh.nnodes))


# ---- the PCG statement ----------------------------------------------------------------------------------------------
def energy_bound(A, free, tol, u_direct):
    """|| u - u_direct ||_A <= tol / sqrt(lambda_min(A_ff)) + cond(A_ff) 2^-52 || u_direct ||_A: the first term from
    || e ||_A^2 = r^T A_ff^-1 r <= || r ||^2 / lambda_min, the second the accuracy of the direct solve itself."""
    Aff = A[free][:, free].toarray()
    lam = np.linalg.eigvalsh(Aff)
    ud = u_direct[free]
    return tol / np.sqrt(lam[0]) + (lam[-1] / lam[0]) * 2.0 ** -52 * np.sqrt(ud @ (Aff @ ud)), Aff


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_pcg_statement_meets_its_stop_rule_and_the_direct_solve(p):
    mesh = create_unit_square(4, shuffle_seed=3, perturb=0.15)
    rng = np.random.default_rng(p)
    kappa = pc.kappa_of(mesh.ncells)
    op = primal.PoissonOperator(mesh, p, kappa)
    op.set_dirichlet(mesh.boundary_facets())
    d = min(p, 3)
    f = rng.standard_normal(mesh.ncells * (d + 1) * (d + 2) // 2)
    b = op.load(d, f)
    u0 = np.where(op.fixed, rng.standard_normal(op.ndofs), 0.0)        # inhomogeneous Dirichlet values
    u, info = op.pcg(b, u0, rtol=1e-10, maxit=2000)
    assert info["converged"] == 1 and info["breakdown"] == 0 and 0 < info["iterations"] < 2000
    tol = 1e-10 * info["nb"]
    assert np.array_equal(u[op.fixed], u0[op.fixed])
    r = op.residual(b, u)
    assert np.sqrt(np.sum(r * r)) <= tol and info["rnorm"] <= tol
    A = pc.assemble(mesh, p, kappa)[0]
    free = np.nonzero(~op.fixed)[0]
    ud = u0.copy()
    ud[free] = spla.spsolve(A[free][:, free].tocsc(), (b - A @ u0)[free])
    bound, Aff = energy_bound(A, free, tol, ud)
    e = (u - ud)[free]
    err = np.sqrt(e @ (Aff @ e))
    print(f"p={p}: {info['iterations']} iterations, energy error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    # the limits
    u3, i3 = op.pcg(b, u0, rtol=1e-10, maxit=3)
    assert i3["converged"] == 0 and i3["iterations"] == 3
    uz, iz = op.pcg(np.zeros(op.ndofs), np.where(op.fixed, 0.0, 1.0), rtol=0.0, atol=0.0, maxit=5)
    assert iz["converged"] == 1 and iz["iterations"] == 0 and np.all(uz == 0.0)


# ---- neumann_load ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_neumann_load_is_the_boundary_integral(p):
    """-int_E g phi_i summed over i is -int_E g (partition of unity); with g the normal component of a constant vector
    over the whole boundary the total vanishes (divergence theorem)."""
    from dolfinx_eqlb_amd.eqlb.bcs import fluxbc
    import galerkin as gk
    mesh = create_unit_square(3, shuffle_seed=1, perturb=0.2)
    sides = gk.side_facets(mesh)
    g = lambda x, y: 1.0 + x * x + 0.0 * y   # noqa: E731
    b = primal.neumann_load(mesh, p, [fluxbc(g, sides[1], scalar=True)])          # y = 0: int_0^1 1 + x^2 = 4/3
    assert abs(b.sum() + 4.0 / 3.0) < 1e-13
    cd = primal.lagrange_dofmap(mesh, p)[0]
    cells = mesh.facet_cells[mesh.facet_cells_offsets[sides[1]]]
    assert set(np.nonzero(b)[0]) <= set(cd[cells].ravel())
    w = lambda x, y: (2.0 + 0.0 * x, -3.0 + 0.0 * y)   # noqa: E731
    b = primal.neumann_load(mesh, p, [fluxbc(w, mesh.boundary_facets()), fluxbc(None, sides[0])])
    assert abs(b.sum()) < 1e-13
    with pytest.raises(ValueError, match="no boundary facet"):
        interior = np.nonzero(np.diff(mesh.facet_cells_offsets) == 2)[0][:1]
        primal.neumann_load(mesh, p, [fluxbc(g, interior, scalar=True)])


# ---- ABI ------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    from dolfinx_eqlb_amd import cpp, lsolver
    header = open(os.path.join(ROOT, "include", "eqlb.h")).read()
    L = cpp.lib()
    for name in ENTRIES:
        assert re.search(r"^int\s+" + name + r"\(", header, flags=re.M), name
        assert name in cpp.EXPORTED_SYMBOLS and hasattr(L, name), name
    assert "eqlb_primal_destroy" in cpp.EXPORTED_SYMBOLS and hasattr(L, "eqlb_primal_destroy")
    for name in ("set_dirichlet", "load", "apply", "diagonal", "residual", "solve"):
        assert hasattr(cpp.PrimalPoisson, name) and hasattr(cpp.PrimalPoisson, name + "_raw"), name
    for name in ("PoissonOperator", "neumann_load", "stiffness_table", "load_table"):
        assert getattr(lsolver, name) is getattr(primal, name)
    from dolfinx_eqlb_amd import _cpp
    for name in ("set_dirichlet", "load", "apply", "diagonal", "residual", "solve"):
        assert hasattr(_cpp.PrimalPoisson, name), name


def test_abi_refuses_bad_arguments_before_the_device():
    from dolfinx_eqlb_amd import cpp
    L = cpp.lib()
    L.eqlb_primal_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int32, C.c_void_p,
                                    C.c_int32, C.c_void_p]
    val = np.full(8, 7.0)
    pv = val.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(0x5EED5EED)   # never dereferenced: the refusal comes first
    host, h = C.c_int32(0), C.c_void_p()

    def refused(st, *words):
        assert st == INVALID_ARGUMENT
        msg = L.eqlb_last_error().decode()
        for w in words:
            assert w in msg, (w, msg)

    for p in (0, 5, -1):
        refused(L.eqlb_primal_create(fake, C.c_int32(p), None, host, None, C.byref(h)), "eqlb_primal_create", "p =")
    refused(L.eqlb_primal_create(None, C.c_int32(2), None, host, None, C.byref(h)), "eqlb_primal_create", "null")
    refused(L.eqlb_primal_create(fake, C.c_int32(2), None, host, None, None), "eqlb_primal_create", "null")
    assert not h
    for d in (-1, 4):
        refused(L.eqlb_primal_load(fake, C.c_int32(d), pv, None, pv, host, None), "eqlb_primal_load", "degree_dg")
    refused(L.eqlb_primal_load(None, C.c_int32(1), pv, None, pv, host, None), "eqlb_primal_load", "null")
    for maxit in (0, -3):
        refused(L.eqlb_primal_solve(fake, pv, pv, 1e-8, 0.0, maxit, pv, 0, None), "eqlb_primal_solve", "maxit")
    for rtol, atol in ((-1e-8, 0.0), (1e-8, -1.0), (float("nan"), 0.0), (0.0, float("nan"))):
        refused(L.eqlb_primal_solve(fake, pv, pv, rtol, atol, 10, pv, 0, None), "eqlb_primal_solve", "rtol")
    refused(L.eqlb_primal_solve(None, pv, pv, 1e-8, 0.0, 10, pv, 0, None), "eqlb_primal_solve", "null")
    refused(L.eqlb_primal_set_dirichlet(fake, C.c_int32(-1), pv, host, None), "eqlb_primal_set_dirichlet", "nlist")
    refused(L.eqlb_primal_set_dirichlet(fake, C.c_int32(2), None, host, None), "eqlb_primal_set_dirichlet", "null")
    refused(L.eqlb_primal_set_dirichlet(None, C.c_int32(1), pv, host, None), "eqlb_primal_set_dirichlet", "null")
    refused(L.eqlb_primal_apply(None, pv, pv, C.c_int32(0), host, None), "eqlb_primal_apply", "null")
    refused(L.eqlb_primal_diagonal(None, pv, host, None), "eqlb_primal_diagonal", "null")
    refused(L.eqlb_primal_residual(None, pv, pv, pv, None, host, None), "eqlb_primal_residual", "null")
    n = C.c_int64(-5)
    refused(L.eqlb_primal_ndofs(None, C.byref(n)), "eqlb_primal_ndofs")
    assert n.value == -5 and np.all(val == 7.0)
    L.eqlb_primal_destroy(None)
    L.eqlb_primal_solve.argtypes = None
