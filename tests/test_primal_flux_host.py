"""Host side of the primal-flux producer (eqlb_primal_flux_dg / eqlb_primal_stress_dg): the tables PG<p,d> compiled
into the library, and the argument errors that are raised before anything is launched.  No device is needed except
where a test says so."""

from fractions import Fraction

import numpy as np
import pytest

from dolfinx_eqlb_amd.elmtlib import polynomials as P
from dolfinx_eqlb_amd.elmtlib.lagrange import Lagrange
from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle

PAIRS = [(p, d) for p in range(1, 5) for d in range(4)]
EPS = np.finfo(np.float64).eps


def _abs_terms(poly, pts):
    """(sum of |c x^a y^b| over the monomials of `poly` at the points, number of monomials): the statement of
    polynomials.evaluate on absolute values."""
    out = np.zeros(pts.shape[0])
    for (a, b), c in poly.items():
        out += abs(float(c)) * np.abs(pts[:, 0]) ** a * np.abs(pts[:, 1]) ** b
    return out, max(len(poly), 1)


def _float_statement(p, d):
    """PG[X][n][i] in floating point and the per-entry tolerance 8 n_terms eps sum|terms| of that statement."""
    el, dg = Lagrange(p), Lagrange(d)
    ders = (P.ddx, P.ddy)
    if d >= p - 1:
        nodes = np.array([[float(a), float(b)] for a, b in dg.nodes])
        tab = el.tabulate(nodes, 1)
        val = np.stack([tab[1], tab[2]])                                   # [X, n, i]
        tol = np.zeros_like(val)
        for X in range(2):
            for i in range(el.ndofs):
                s, nt = _abs_terms(ders[X](el.basis[i]), nodes)
                tol[X, :, i] = 8 * nt * EPS * s
        return val, tol
    qp, qw = make_quadrature_triangle(2 * p + 2)
    psi = dg.tabulate(qp)[0]                                               # [q, n]
    tab = el.tabulate(qp, 1)
    minv = np.linalg.inv(np.einsum("q,qn,qm->nm", qw, psi, psi))
    val = np.stack([minv @ np.einsum("q,qm,qi->mi", qw, psi, tab[1 + X]) for X in range(2)])
    absum = np.stack([np.abs(minv) @ np.einsum("q,qm,qi->mi", qw, np.abs(psi), np.abs(tab[1 + X]))
                      for X in range(2)])
    return val, 8 * (dg.ndofs * qw.size) * EPS * absum


@pytest.mark.parametrize("p,d", PAIRS)
def test_table_equals_float_quadrature_statement(p, d):
    from dolfinx_eqlb_amd import cpp
    got = cpp.get_primal_table(p, d)
    val, tol = _float_statement(p, d)
    assert got.shape == val.shape == (2, (d + 1) * (d + 2) // 2, (p + 1) * (p + 2) // 2)
    err = np.abs(got - val)
    print(f"p={p} d={d}: max err {err.max():.3e}, smallest tolerance margin {(tol - err).min():.3e}")
    assert (err <= tol).all()
    assert np.abs(got).max() > 0.5  # not an empty table


@pytest.mark.parametrize("p,d", [(p, d) for (p, d) in PAIRS if d >= p - 1])
def test_table_equals_exact_tabulation(p, d):
    """d >= p-1: the entries are the exact rational values of d/dX phi_i at the DG_d nodes, rounded once."""
    from dolfinx_eqlb_amd import cpp
    el, dg = Lagrange(p), Lagrange(d)
    exact = np.array([[[float(sum((c * x ** a * y ** b for (a, b), c in der(el.basis[i]).items()), Fraction(0)))
                        for i in range(el.ndofs)] for (x, y) in dg.nodes] for der in (P.ddx, P.ddy)])
    assert np.array_equal(cpp.get_primal_table(p, d), exact)


@pytest.mark.parametrize("p,d", PAIRS)
def test_table_equals_generator(p, d):
    from dolfinx_eqlb_amd import cpp
    from gen_tables import primal_table_float
    assert np.array_equal(cpp.get_primal_table(p, d), primal_table_float(p, d))


class _NoMesh:
    _h = None


@pytest.mark.parametrize("p,d", [(0, 0), (5, 1), (2, -1), (2, 4)])
def test_bad_degrees_raise(p, d):
    from dolfinx_eqlb_amd import cpp
    cd, u, out = np.zeros((1, 15), np.int32), np.zeros(4), np.zeros(64)
    with pytest.raises(RuntimeError, match="outside"):
        cpp.primal_flux_dg_raw(_NoMesh, p, d, 1, cd.ctypes.data, 4, u.ctypes.data, None, out.ctypes.data,
                               memspace=cpp.MEM_HOST)
    with pytest.raises(RuntimeError, match="outside"):
        cpp.primal_stress_dg_raw(_NoMesh, p, d, cd.ctypes.data, 2, u.ctypes.data, 1.0, None, out.ctypes.data,
                                 memspace=cpp.MEM_HOST)
    with pytest.raises(RuntimeError, match="outside"):
        cpp.get_primal_table(p, d)
    assert (out == 0).all()


def test_nrhs_zero_raises():
    from dolfinx_eqlb_amd import cpp
    cd, u, out = np.zeros((1, 6), np.int32), np.zeros(4), np.zeros(64)
    with pytest.raises(RuntimeError, match="nrhs"):
        cpp.primal_flux_dg_raw(_NoMesh, 2, 1, 0, cd.ctypes.data, 4, u.ctypes.data, None, out.ctypes.data,
                               memspace=cpp.MEM_HOST)


def test_local_projection_wrong_size_raises():
    from dolfinx_eqlb_amd.lsolver import PrimalFlux, PrimalStress, local_projection
    from dolfinx_eqlb_amd.mesh import create_unit_square
    mesh = create_unit_square(2)
    cd = np.zeros((mesh.ncells, 6), np.int32)
    with pytest.raises(RuntimeError, match="Input sizes does not match"):
        local_projection(mesh, 1, [PrimalFlux(np.zeros(30), cd[:, :5], 2)], bs=2)
    with pytest.raises(RuntimeError, match="Input sizes does not match"):
        local_projection(mesh, 1, [PrimalFlux(np.zeros(30), cd, 2)], bs=1)
    with pytest.raises(RuntimeError, match="Input sizes does not match"):
        local_projection(mesh, 1, [PrimalStress(np.zeros(31), cd, 2, 1.0, 0)], bs=2)


def test_out_of_range_index_in_host_memory_raises():
    from dolfinx_eqlb_amd import cpp
    if cpp.device_count() == 0:
        pytest.skip("needs a device: the mesh handle lives there")
    from dolfinx_eqlb_amd.mesh import create_unit_square
    from galerkin import dofmap
    mesh = create_unit_square(2)
    dm = cpp.DeviceMesh(mesh)
    cd, ndofs = dofmap(mesh, 2)
    u = np.ones(ndofs)
    for bad in (-1, ndofs):
        cdb = cd.copy()
        cdb[3, 2] = bad
        with pytest.raises(RuntimeError, match=r"cell_dofs\[3\]\[2\]"):
            cpp.primal_flux_dg(dm, 2, 1, cdb, u)
        with pytest.raises(RuntimeError, match=r"cell_dofs\[3\]\[2\]"):
            cpp.primal_stress_dg(dm, 2, 1, cdb, np.ones((ndofs, 2)))
