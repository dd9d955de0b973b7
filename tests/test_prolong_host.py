"""The numpy statement of the transfer across a refinement (dolfinx_eqlb_amd/mesh/transfer.py) and the table the
library carries for it, without a device: the dofmap against tests/galerkin.py, the table bit for bit, its exact
properties, and polynomial reproduction of P_p and DG_d on refined meshes."""

from fractions import Fraction

import numpy as np
import pytest

from refine_cases import case

EPS = np.finfo(np.float64).eps
_REFINED = {}


def refined(name):
    """(mesh, mesh2, parent_cell, node_parent_facet) of a case of tests/refine_cases.py, by the statement."""
    if name not in _REFINED:
        from dolfinx_eqlb_amd.mesh import create_mesh, refine_longest_edge
        mesh, marked = case(name)
        x2, c2, pc, npf = refine_longest_edge(mesh, marked)
        _REFINED[name] = (mesh, create_mesh(x2, c2), pc, npf)
    return _REFINED[name]


@pytest.mark.parametrize("name", ["sq3_cell5", "hole"])
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_lagrange_dofmap_is_the_dofmap_of_the_test_solver(name, p):
    from galerkin import dofmap
    from dolfinx_eqlb_amd.mesh import lagrange_dofmap
    mesh = case(name)[0]
    cd, n = lagrange_dofmap(mesh, p)
    ref, nref = dofmap(mesh, p)
    assert cd.dtype == np.int32 and cd.shape == ref.shape and n == nref
    assert np.array_equal(cd, ref)


@pytest.mark.parametrize("q", [1, 2, 3, 4])
def test_library_table_is_the_statement_bit_for_bit(q):
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.mesh import prolong_table
    T = prolong_table(q)
    assert T.shape == ((2 * q + 1) * (2 * q + 2) // 2, (q + 1) * (q + 2) // 2)
    got = cpp.get_prolong_table(q)
    assert got.shape == T.shape and np.array_equal(got.view(np.int64), T.view(np.int64))


@pytest.mark.parametrize("q", [1, 2, 3, 4])
def test_rows_sum_to_one_and_even_points_are_unit_rows(q):
    from dolfinx_eqlb_amd.elmtlib.lagrange import lagrange_nodes
    from dolfinx_eqlb_amd.mesh.transfer import lattice_row, prolong_table, prolong_table_exact
    T = prolong_table_exact(q)
    assert all(isinstance(v, Fraction) for row in T for v in row)
    assert all(sum(row) == 1 for row in T)
    # the row order covers 0 ... nrow - 1 once
    rows = [lattice_row(q, i, j) for j in range(2 * q + 1) for i in range(2 * q + 1 - j)]
    assert rows == list(range(len(T)))
    # an even lattice point is a node of P_q: its row is the unit vector of that node
    Tf = prolong_table(q)
    for k, (x, y) in enumerate(lagrange_nodes(q)):
        r = lattice_row(q, int(2 * q * x), int(2 * q * y))
        unit = np.zeros(len(T[0]))
        unit[k] = 1.0
        assert np.array_equal(Tf[r], unit), (q, k)
    even = sum(1 for j in range(0, 2 * q + 1, 2) for i in range(0, 2 * q + 1 - j, 2))
    assert even == len(T[0])


def test_library_table_refusals():
    import ctypes as C
    from dolfinx_eqlb_amd import cpp
    L = cpp.lib()
    out = np.full(4, 7.0)
    for q in (0, 5, -1):
        assert L.eqlb_get_prolong_table(C.c_int32(q), out.ctypes.data_as(C.c_void_p), C.c_int32(4)) < 0
        assert "eqlb_get_prolong_table" in L.eqlb_last_error().decode()
    assert L.eqlb_get_prolong_table(C.c_int32(1), out.ctypes.data_as(C.c_void_p), C.c_int32(4)) < 0   # needs 18
    assert L.eqlb_get_prolong_table(C.c_int32(1), None, C.c_int32(100)) < 0
    assert np.all(out == 7.0)


def _poly(deg, x, y):
    """A polynomial of total degree `deg` with all monomials, values of order one on the unit square."""
    return sum((0.3 + 0.1 * a + 0.07 * b) * x ** a * y ** b for a in range(deg + 1) for b in range(deg + 1 - a))


def _dof_points(mesh, q):
    """Physical points of the local DOFs of P_q / DG_q on every cell [ncells, nd, 2]."""
    from dolfinx_eqlb_amd.elmtlib.lagrange import lagrange_nodes
    nodes = np.array([[float(a), float(b)] for a, b in lagrange_nodes(q)])
    X = mesh.x[mesh.cell_nodes, :2]
    return X[:, None, 0] + nodes[None, :, 0:1] * (X[:, 1] - X[:, 0])[:, None] \
        + nodes[None, :, 1:2] * (X[:, 2] - X[:, 0])[:, None]


@pytest.mark.parametrize("name", ["triangle", "right1", "sq3_all", "disk"])
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_lagrange_prolongation_reproduces_polynomials(name, p):
    """The interpolant of a polynomial f of total degree p is f itself on every cell, so its prolongation is the
    interpolant on the refined mesh.  Bound: the exact value at a child DOF is sum_i T_exact[r][i] f(x_i); the
    statement uses T rounded once (relative eps/2 per entry), values f(x_i) rounded by their evaluation, and adds nd
    products (nd * eps/2 each way to first order): |error| <= c eps A with A = sum_i |T[r][i]| |v_i| and c = 2 nd -
    the bound of the device tests, which also covers the evaluation error of f at the two point sets (a few eps of
    |f| <= A, since the rows sum to one)."""
    from dolfinx_eqlb_amd.mesh import lagrange_dofmap, prolong_lagrange
    mesh, mesh2, pc, npf = refined(name)
    nd = (p + 1) * (p + 2) // 2

    def interpolant(m):
        cd, n = lagrange_dofmap(m, p)
        pts = _dof_points(m, p)
        u = np.zeros(n)
        u[cd] = _poly(p, pts[..., 0], pts[..., 1])
        return u

    u, want = interpolant(mesh), interpolant(mesh2)
    for bs in (1, 2):
        ub = np.stack([u * (1 + b) for b in range(bs)], axis=1).reshape(1, -1)
        got, A = prolong_lagrange(mesh, mesh2, pc, npf, p, ub, bs=bs, return_abs=True)
        for b in range(bs):
            err = np.abs(got[0, b::bs] - want * (1 + b))
            ratio = (err / (EPS * A[0, b::bs])).max()
            assert ratio <= 2 * nd, (name, p, bs, ratio)


@pytest.mark.parametrize("name", ["triangle", "right1", "sq3_all", "disk"])
@pytest.mark.parametrize("d", [0, 1, 2, 3])
def test_dg_prolongation_reproduces_polynomials(name, d):
    """As above for DG_d nodal values of a polynomial of total degree d (d = 0: the constant), same bound."""
    from dolfinx_eqlb_amd.mesh import prolong_dg
    mesh, mesh2, pc, npf = refined(name)
    nd = (d + 1) * (d + 2) // 2

    def values(m):
        pts = _dof_points(m, d)
        return _poly(d, pts[..., 0], pts[..., 1]).reshape(-1)

    v, want = values(mesh), values(mesh2)
    for bs in (1, 2):
        vb = np.stack([v * (1 + b) for b in range(bs)], axis=1).reshape(1, -1)
        got, A = prolong_dg(mesh, mesh2, pc, npf, d, vb, bs=bs, return_abs=True)
        assert got.shape == (1, mesh2.ncells * nd * bs)
        for b in range(bs):
            err = np.abs(got[0, b::bs] - want * (1 + b))
            assert (err / (EPS * A[0, b::bs])).max() <= 2 * nd, (name, d, bs)


def test_copied_cells_and_old_nodes_keep_their_values_bit_for_bit():
    from dolfinx_eqlb_amd.mesh import lagrange_dofmap, prolong_dg, prolong_lagrange
    mesh, mesh2, pc, npf = refined("sq3_cell5")
    copied = np.nonzero(np.bincount(pc, minlength=mesh.ncells)[pc] == 1)[0]
    assert 0 < copied.size < mesh2.ncells
    rng = np.random.default_rng(3)
    for p in (1, 3):
        cd, n = lagrange_dofmap(mesh, p)
        cd2, n2 = lagrange_dofmap(mesh2, p)
        u = rng.standard_normal((2, n))
        u2 = prolong_lagrange(mesh, mesh2, pc, npf, p, u)
        assert u2.shape == (2, n2)
        assert np.array_equal(u2[:, :mesh.nnodes], u[:, :mesh.nnodes])
        assert np.array_equal(u2[:, cd2[copied]], u[:, cd[pc[copied]]])
    v = rng.standard_normal((1, mesh.ncells * 6 * 2))
    v2 = prolong_dg(mesh, mesh2, pc, npf, 2, v, bs=2)
    assert np.array_equal(v2.reshape(mesh2.ncells, 12)[copied], v.reshape(mesh.ncells, 12)[pc[copied]])
