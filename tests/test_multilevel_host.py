"""The multilevel preconditioner of the P_p solves as far as it can be checked without a device: the numpy statements
(mesh.transfer.restrict_lagrange, lsolver.multilevel.Hierarchy) against the transpose of the prolongation built as a
dense matrix, the preconditioner as a dense matrix (symmetric, zero on the fixed rows, positive definite on the free
ones), Hierarchy.pcg against a direct solve and against the Jacobi statement, and the refusals of the C ABI that need no
mesh.

The mesh create_unit_square(3, shuffle_seed=3, perturb=0.15) has 36 cells; refined at refine_cases.level_marks it has
parents with 1, 2, 3 and 4 children."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import elasticity_cases as ec
import multilevel_cases as mc
import primal_cases as pc
from dolfinx_eqlb_amd.mesh import create_unit_square
from dolfinx_eqlb_amd.mesh import transfer as tr
from refine_cases import level_marks

U = pc.U
INVALID_ARGUMENT = -1
ENTRIES = ("eqlb_hierarchy_create", "eqlb_hierarchy_restrict", "eqlb_hierarchy_precondition", "eqlb_hierarchy_solve")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def levels(last="partial"):
    """three levels: 36 cells, refined at level_marks(., 1) (45 cells), then at level_marks(., 2) (the dense matrices) or
    uniformly (180 cells: the smallest of these hierarchies on which Jacobi is not finished by the small dimension)"""
    if last not in _CACHE:
        base = create_unit_square(3, shuffle_seed=3, perturb=0.15)
        second = (lambda n: level_marks(n, 2)) if last == "partial" else mc.all_cells
        _CACHE[last] = mc.levels_host(base, [lambda n: level_marks(n, 1), second])
    return _CACHE[last]


# ---- 1. the restriction is the transpose of the prolongation -----------------------------------------------------------
@pytest.mark.parametrize("bs", [1, 2])
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_restriction_is_the_transpose(p, bs):
    meshes, links = levels()
    mesh, mesh2 = meshes[0], meshes[1]
    pcell, npf = links[0]
    assert sorted(set(np.bincount(pcell, minlength=mesh.ncells))) == [1, 2, 3, 4]
    mc.check_restriction(mesh, mesh2, pcell, npf, p, bs)


def test_restriction_refuses_bad_input():
    meshes, links = levels()
    pcell, npf = links[0]
    with pytest.raises(ValueError, match="p = 5"):
        tr.restrict_lagrange(meshes[0], meshes[1], pcell, npf, 5, np.zeros(3))
    with pytest.raises(ValueError, match="side by side"):
        tr.restrict_lagrange(meshes[0], meshes[1], pcell[::-1], npf, 1, np.zeros(meshes[1].nnodes))
    from dolfinx_eqlb_amd import mesh as mesh_pkg
    assert mesh_pkg.restrict_lagrange is tr.restrict_lagrange


# ---- 2. the preconditioner as a dense matrix ------------------------------------------------------------------------
def dense_preconditioner(H):
    n = H.ops[-1].fixed.size
    return np.stack([H.precondition(e) for e in np.eye(n)], axis=1)


def abs_preconditioner(H):
    """the recursion of the statement with absolute values: F (|P| M |P|^T + D^-1) F"""
    bs = H.bs
    M = None
    for l, op in enumerate(H.ops):
        free = (~op.fixed).astype(np.float64)
        D = np.diag(1.0 / np.abs(H.diag(l)))
        if M is not None:
            pcell, npf = H.links[l - 1]
            P = np.kron(np.abs(mc.dense_prolongation(H.ops[l - 1].mesh, op.mesh, pcell, npf, H.p)), np.eye(bs))
            D = P @ M @ P.T + D
        M = free[:, None] * D * free[None, :]
    return M


@pytest.mark.parametrize("problem,p", [("poisson", 1), ("poisson", 2), ("elasticity", 1), ("elasticity", 2)])
def test_preconditioner_is_symmetric_positive_definite(problem, p):
    meshes, links = levels()
    H, _ = mc.hierarchy(meshes, links, p, problem)
    assert H.nlevels == 3 and H.ops[-1].fixed.size <= 600
    M = dense_preconditioner(H)
    fixed = H.ops[-1].fixed
    assert np.all(M[fixed] == 0.0) and np.all(M[:, fixed] == 0.0)
    # every level adds the roundings of one restriction and one prolongation (nd_p) and three single operations to either
    # of the two entries compared
    nd = (p + 1) * (p + 2) // 2
    terms = 2 * sum(mc.restrict_terms(m, p)[0] + nd + 3 for m in meshes)
    Mabs = abs_preconditioner(H)
    asym = np.abs(M - M.T)
    print(f"{problem} p={p}: {fixed.size} rows, max asymmetry / (2^-53 abs-sum) "
          f"{np.max(asym[Mabs > 0] / (U * Mabs[Mabs > 0])):.2f}, allowed {terms}")
    assert np.all(asym <= terms * U * Mabs)
    lam = np.linalg.eigvalsh(0.5 * (M + M.T)[~fixed][:, ~fixed])
    print(f"eigenvalues of the free block: {lam[0]:.3e} ... {lam[-1]:.3e}")
    assert lam[0] > 0.0


def test_one_level_is_jacobi():
    meshes, _ = levels()
    op = mc.poisson_op(meshes[0], 2, pc.kappa_of(meshes[0].ncells))
    H = mc.Hierarchy([op], [])
    r = np.random.default_rng(4).standard_normal(op.ndofs)
    assert np.array_equal(H.precondition(r), np.where(op.fixed, 0.0, r / op.diagonal()))
    with pytest.raises(ValueError, match="different p"):
        mc.Hierarchy([op, mc.poisson_op(meshes[1], 1, None)], [levels()[1][0]])
    with pytest.raises(ValueError, match="level = 0"):
        H.restrict(0, r)


# ---- 3. Hierarchy.pcg -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem,p", [("poisson", 1), ("poisson", 2), ("poisson", 3), ("poisson", 4),
                                        ("elasticity", 1), ("elasticity", 2)])
def test_pcg_against_a_direct_solve_and_against_jacobi(problem, p):
    """the bounds of check_solution of the device tests; fewer iterations than the Jacobi statement"""
    meshes, links = levels("uniform")
    assert [m.ncells for m in meshes] == [36, 45, 180]
    rng = np.random.default_rng(7 * p)
    H, coeff = mc.hierarchy(meshes, links, p, problem)
    if problem == "poisson":
        from test_gpu_primal_solve import check_solution
        A = pc.assemble(meshes[-1], p, coeff[-1])[0]
    else:
        from test_gpu_primal_elasticity import check_solution
        A = ec.assemble(meshes[-1], p, 1.0, coeff[-1])[0]
    op = H.ops[-1]
    n = op.fixed.size
    b = rng.standard_normal(n)
    u0 = np.where(op.fixed, rng.standard_normal(n), 0.0)
    u, info = H.pcg(b, u0, rtol=1e-10, maxit=5000)
    check_solution(op, A, b, u0, u, info, 1e-10)
    _, jac = op.pcg(b, u0, rtol=1e-10, maxit=5000)
    print(f"{problem} p={p}: hierarchy {info['iterations']} iterations, Jacobi {jac['iterations']}")
    assert jac["converged"] == 1 and info["iterations"] < jac["iterations"]


def test_pcg_limits():
    meshes, links = levels()
    H, _ = mc.hierarchy(meshes, links, 2, "poisson")
    op = H.ops[-1]
    b = np.random.default_rng(1).standard_normal(op.ndofs)
    u0 = np.zeros(op.ndofs)
    _, i3 = H.pcg(b, u0, rtol=1e-10, maxit=3)
    assert i3["iterations"] == 3 and i3["converged"] == 0 and i3["breakdown"] == 0
    bn = b.copy()
    bn[np.nonzero(~op.fixed)[0][3]] = np.nan
    _, i4 = H.pcg(bn, u0, rtol=1e-10, maxit=40)
    assert i4["breakdown"] == 1 and i4["converged"] == 0
    u5, i5 = H.pcg(np.zeros(op.ndofs), np.where(op.fixed, 0.0, 1.0), rtol=0.0, atol=0.0, maxit=5)
    assert i5["converged"] == 1 and i5["iterations"] == 0 and np.all(u5 == 0.0)


def test_growth_with_the_level_of_the_statement():
    """P_1 on uniformly refined levels of create_unit_square(2, ...), 16 * 4^L cells: from L = 3 to L = 5 the count of
    the hierarchy grows by at most 1.5, that of Jacobi by at least 2 - the margins of the device test, on the statement"""
    base = create_unit_square(2, shuffle_seed=3, perturb=0.15)
    meshes, links = mc.levels_host(base, [mc.all_cells] * 5)
    counts = {}
    for L in (3, 5):
        H = mc.Hierarchy([mc.poisson_op(m, 1, None) for m in meshes[:L + 1]], links[:L])
        op = H.ops[-1]
        b = np.random.default_rng(L).standard_normal(op.ndofs)
        u0 = np.zeros(op.ndofs)
        counts[L] = (H.pcg(b, u0, rtol=1e-8, maxit=5000)[1]["iterations"], op.pcg(b, u0, rtol=1e-8, maxit=5000)[1]["iterations"])
        print(f"L = {L}: {op.mesh.ncells} cells, hierarchy {counts[L][0]} iterations, Jacobi {counts[L][1]}")
    assert counts[5][0] <= 1.5 * counts[3][0]
    assert counts[5][1] >= 2 * counts[3][1]


# ---- 4. the C ABI without a device ---------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    from dolfinx_eqlb_amd import cpp
    header = open(os.path.join(ROOT, "include", "eqlb.h")).read()
    L = cpp.lib()
    for name in ENTRIES:
        assert re.search(r"^int\s+" + name + r"\(", header, flags=re.M), name
        assert name in cpp.EXPORTED_SYMBOLS, name
        assert hasattr(L, name), name
    assert re.search(r"^void\s+eqlb_hierarchy_destroy\(", header, flags=re.M)
    assert "eqlb_hierarchy_destroy" in cpp.EXPORTED_SYMBOLS and hasattr(L, "eqlb_hierarchy_destroy")
    for name in ("restrict", "restrict_raw", "precondition", "precondition_raw", "solve", "solve_raw", "close"):
        assert hasattr(cpp.Multilevel, name), name
    from dolfinx_eqlb_amd import _cpp
    for name in ("restrict", "precondition", "solve"):
        assert hasattr(_cpp.Multilevel, name), name
    from dolfinx_eqlb_amd import lsolver
    from dolfinx_eqlb_amd.lsolver import multilevel
    assert lsolver.Hierarchy is multilevel.Hierarchy


def test_refusals_that_need_no_mesh():
    """refused by name before anything is dereferenced or launched; the outputs stay as they were"""
    from dolfinx_eqlb_amd import cpp
    L = cpp.lib()
    val = np.full(12, 7.0)
    pv = val.ctypes.data_as(C.c_void_p)
    host, one = C.c_int32(0), C.c_int32(1)
    fake = C.c_void_p(0x5EED5EED)   # never dereferenced: the refusal comes first
    ptrs = (C.c_void_p * 1)(fake)
    out = C.c_void_p(0x1234)
    create = L.eqlb_hierarchy_create
    for nlev, bs, sv, pl, ms, o, word in ((0, 1, ptrs, ptrs, ptrs, C.byref(out), "nlevels"),
                                          (-3, 2, ptrs, ptrs, ptrs, C.byref(out), "nlevels"),
                                          (1, 3, ptrs, ptrs, ptrs, C.byref(out), "bs = 3"),
                                          (1, 0, ptrs, ptrs, ptrs, C.byref(out), "bs = 0"),
                                          (1, 1, None, ptrs, ptrs, C.byref(out), "null"),
                                          (1, 1, ptrs, ptrs, None, C.byref(out), "null"),
                                          (1, 1, ptrs, ptrs, ptrs, None, "null"),
                                          (2, 1, (C.c_void_p * 2)(fake, fake), None, (C.c_void_p * 2)(fake, fake),
                                           C.byref(out), "null"),
                                          (2, 1, (C.c_void_p * 2)(fake, None), (C.c_void_p * 1)(fake),
                                           (C.c_void_p * 2)(fake, fake), C.byref(out), "null"),
                                          (1, 2, (C.c_void_p * 1)(None), ptrs, ptrs, C.byref(out), "null")):
        assert create(C.c_int32(nlev), C.c_int32(bs), sv, pl, ms, None, o) == INVALID_ARGUMENT
        msg = L.eqlb_last_error().decode()
        assert "eqlb_hierarchy_create" in msg and word in msg, msg
        assert out.value == 0x1234
    assert L.eqlb_hierarchy_restrict(None, C.c_int32(0), pv, pv, one, host, None) == INVALID_ARGUMENT
    assert "eqlb_hierarchy_restrict" in L.eqlb_last_error().decode()
    assert L.eqlb_hierarchy_precondition(None, pv, pv, host, None) == INVALID_ARGUMENT
    assert "eqlb_hierarchy_precondition" in L.eqlb_last_error().decode()
    info = (C.c_double * 8)(*([5.0] * 8))
    for h, b, u, i, maxit, rtol in ((None, pv, pv, info, 10, 1e-8), (fake, None, pv, info, 10, 1e-8),
                                    (fake, pv, None, info, 10, 1e-8), (fake, pv, pv, None, 10, 1e-8),
                                    (fake, pv, pv, info, 0, 1e-8), (fake, pv, pv, info, 10, -1.0),
                                    (fake, pv, pv, info, 10, float("nan"))):
        st = L.eqlb_hierarchy_solve(h, b, u, C.c_double(rtol), C.c_double(0.0), C.c_int32(maxit), i, host, None)
        assert st == INVALID_ARGUMENT and "eqlb_hierarchy_solve" in L.eqlb_last_error().decode()
    assert np.all(val == 7.0) and list(info) == [5.0] * 8
    L.eqlb_hierarchy_destroy(None)   # as free(NULL)


def test_binding_refuses_what_it_can_see():
    from dolfinx_eqlb_amd import cpp
    with pytest.raises(RuntimeError, match="one Refinement per pair"):
        cpp.Multilevel([], [])
    with pytest.raises(RuntimeError, match="PrimalPoisson handles or PrimalElasticity handles"):
        cpp.Multilevel([object()], [])
