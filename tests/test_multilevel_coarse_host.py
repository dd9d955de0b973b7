"""The exact solve on level 0 of the multilevel preconditioner (lsolver.multilevel.Hierarchy(..., coarse=True)) as far as
it can be checked without a device: the operator of level 0 from apply is symmetric (exactly, but for the elasticity
statement on a mesh with general coordinates: test_level0_operator_is_symmetric), the LDL^T factor of the
statement against numpy within a bound counted from its roundings, the preconditioner as a dense matrix (symmetric
within rounding, positive definite on the free rows), the switch off (the bits of the rule without it), the iteration
counts on the graded hierarchy from create_unit_square(8), the refusals, and the new entries of the C ABI as far as
they need no mesh.

The small hierarchy is that of tests/test_multilevel_host.py: create_unit_square(3, shuffle_seed=3, perturb=0.15) with
36 cells, refined at refine_cases.level_marks."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import multilevel_cases as mc
import multilevel_local_cases as lc
import primal_cases as pc
import primal_mesh_cases as pm
from dolfinx_eqlb_amd.lsolver.multilevel import Hierarchy
from dolfinx_eqlb_amd.mesh import create_unit_square
from refine_cases import level_marks

U = pc.U
INVALID_ARGUMENT = -1
NEW_ENTRIES = ("eqlb_hierarchy_set_coarse", "eqlb_hierarchy_coarse_rows", "eqlb_hierarchy_coarse_factor")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def levels():
    """three levels: 36 cells, refined at level_marks(., 1), then at level_marks(., 2)"""
    if "levels" not in _CACHE:
        base = create_unit_square(3, shuffle_seed=3, perturb=0.15)
        _CACHE["levels"] = mc.levels_host(base, [lambda n: level_marks(n, 1), lambda n: level_marks(n, 2)])
    return _CACHE["levels"]


def graded8(nref=6):
    """create_unit_square(8) (256 cells) and `nref` graded refinements (multilevel_local_cases.graded_marks)"""
    if "graded8" not in _CACHE:
        meshes, links = [create_unit_square(8)], []
        for _ in range(nref):
            m2, pcell, npf = mc.refine_host(meshes[-1], lc.graded_marks(meshes[-1]))
            meshes.append(m2)
            links.append((pcell, npf))
        _CACHE["graded8"] = (meshes, links)
    return _CACHE["graded8"]


def variants(meshes, links, p, problem):
    """{(local, coarse): Hierarchy} on the same operators"""
    H, _ = mc.hierarchy(meshes, links, p, problem)
    return {(lo, co): Hierarchy(H.ops, H.links, local=lo, coarse=co) for lo in (False, True) for co in (False, True)}


def level0_cases():
    """name -> Hierarchy(coarse=True) whose level 0 is checked"""
    if "level0" not in _CACHE:
        meshes, links = levels()
        out = {}
        for problem, p in (("poisson", 1), ("poisson", 2), ("elasticity", 1), ("elasticity", 2)):
            out[f"{problem}-p{p}"] = variants(meshes, links, p, problem)[(False, True)]
        op = pm.statement("poisson", pm.mesh_of("aspect1000"), 1, "all")[0]
        out["poisson-p1-aspect1000"] = Hierarchy([op], [], coarse=True)
        _CACHE["level0"] = out
    return _CACHE["level0"]


LEVEL0 = ["poisson-p1", "poisson-p2", "elasticity-p1", "elasticity-p2", "poisson-p1-aspect1000"]


# ---- 1. the matrix of level 0 ------------------------------------------------------------------------------------------
def level0_matrix(H):
    rows, A = H.coarse_matrix()
    assert rows.dtype == np.int32 and np.array_equal(rows, np.nonzero(~H.ops[0].fixed)[0])
    assert A.shape == (rows.size, rows.size) and rows.size > 0
    assert np.all(np.diag(A) > 0.0)
    return rows, A


@pytest.mark.parametrize("name", LEVEL0)
def test_level0_operator_is_symmetric(name):
    """The Poisson statement forms a_ij and a_ji of a cell by the same operations on a symmetric table and adds the
    cells in the same order: A_0 is exactly symmetric on any mesh.  The elasticity statement forms the two off-diagonal
    blocks of a cell in different orders, so on a mesh with general coordinates a_ij and a_ji differ in the last bits
    (2.7e-15 on level 0 here at P_1): there the two are within the roundings of their chains (elasticity_cases.chain_terms
    against the abs-sums of apply), and the rule reads the lower triangle only.  On the unperturbed create_unit_square
    meshes, whose coordinates are dyadic, it is exact as well: the next test."""
    H = level0_cases()[name]
    rows, A = level0_matrix(H)
    asym = np.abs(A - A.T)
    print(f"{name}: n = {rows.size}, max |A - A^T| = {np.max(asym)}")
    if H.bs == 1:
        assert np.array_equal(A, A.T)
        return
    op = H.ops[0]
    Aabs = np.zeros_like(A)
    e = np.zeros(op.fixed.size)
    for j, row in enumerate(rows):
        e[row] = 1.0
        Aabs[:, j] = op.apply(e, masked=True, return_abs=True)[1][rows]
        e[row] = 0.0
    terms = pm.ec.chain_terms(H.p, pm.valence(op.mesh), 0)[0]
    bound = terms * U * (Aabs + Aabs.T)
    print(f"max asymmetry / bound {pc.ratio(asym, bound):.3f} ({terms} roundings per entry)")
    assert np.all(asym <= bound)


@pytest.mark.parametrize("problem,p", [("poisson", 1), ("elasticity", 1), ("poisson", 2)])
def test_level0_operator_is_exactly_symmetric_on_the_unit_square(problem, p):
    """level 0 of the hierarchy of the iteration counts: create_unit_square(8)"""
    mesh = graded8()[0][0]
    H, _ = mc.hierarchy([mesh], [], p, problem)
    rows, A = level0_matrix(H)
    assert rows.size == {("poisson", 1): 113, ("elasticity", 1): 226, ("poisson", 2): 481}[(problem, p)]
    assert np.array_equal(A, A.T)


# ---- 2. the factor against numpy ---------------------------------------------------------------------------------------
def factor_bounds(A, d, W):
    """Entrywise bounds, counted as primal_cases.chain_terms counts: every rounding of the longest chain of an entry is
    bounded by 2^-53 of the abs-sum of the computation it belongs to.  With L = W^-1 and the abs-sum S = |L| D |L|^T:
      the elimination   an entry a_ij takes at most n steps of one product and one difference, and one division forms
                        l: 2 n + 1 roundings against S - the computed factor is the exact factor of A + E, |E| <= (2 n + 1) u S
      W                 an entry w_ij takes at most n steps of one product and one difference: 2 n roundings against
                        |L| |W|, so L W = I + F with |F| <= 2 n u |L| |W|, and L differs from W^-1 by F L
    Together A - W^-1 D W^-T = G with |G| <= u ((2 n + 1) S + 2 n (|L| |W| S + its transpose)).
      W A W^T - D       = W G W^T; the two numpy products that evaluate it add n + 1 roundings each against |W| |A| |W|^T
      M_0 - A^-1        = A^-1 G M_0 (M_0 = W^T D^-1 W exactly); the two passes of coarse_solve add n products, n sums
                        and the division, each pass against |W|^T D^-1 |W|: 2 (2 n + 1); numpy's inverse (LU, backward
                        error 3 n u |L_lu| |U_lu|, which for this matrix is S up to the pivoting) adds
                        3 n u |A^-1| S |A^-1|
    Returns (bound of W A W^T - D, bound of M_0 - A^-1)."""
    n = d.size
    L = np.linalg.inv(W)
    aL, aW = np.abs(L), np.abs(W)
    S = aL @ np.diag(d) @ aL.T
    T = aL @ aW @ S
    G = U * ((2 * n + 1) * S + 2 * n * (T + T.T))
    b1 = aW @ G @ aW.T + 2 * (n + 1) * U * (aW @ np.abs(A) @ aW.T)
    Ainv = np.abs(np.linalg.inv(A))
    Mabs = aW.T @ np.diag(1.0 / d) @ aW
    b2 = Ainv @ G @ Mabs + 2 * (2 * n + 1) * U * Mabs + 3 * n * U * (Ainv @ S @ Ainv)
    return b1, b2


@pytest.mark.parametrize("name", LEVEL0)
def test_factor_against_numpy(name):
    H = level0_cases()[name]
    rows, A = H.coarse_matrix()
    rows2, d, W = H.coarse_factor()
    n = rows.size
    assert np.array_equal(rows2, rows) and rows2.dtype == np.int32 and d.shape == (n,) and W.shape == (n, n)
    assert np.all(d > 0.0) and np.all(np.diag(W) == 1.0) and np.all(np.triu(W, 1) == 0.0)
    b1, b2 = factor_bounds(A, d, W)
    dev1 = np.abs(W @ A @ W.T - np.diag(d))
    # M_0 as the statement applies it: column by column through coarse_solve
    e = np.zeros(H.ops[0].fixed.size)
    M0 = np.zeros((n, n))
    for j, row in enumerate(rows):
        e[row] = 1.0
        z = H.coarse_solve(e)
        e[row] = 0.0
        assert np.all(z[H.ops[0].fixed] == 0.0)
        M0[:, j] = z[rows]
    dev2 = np.abs(M0 - np.linalg.inv(A))
    print(f"{name}: n = {n}, cond {np.linalg.cond(A):.2e}; W A W^T - D: max deviation / bound {pc.ratio(dev1, b1):.3f}; "
          f"M_0 - inv(A): max deviation / bound {pc.ratio(dev2, b2):.3f}, relative {np.max(dev2) / np.max(np.abs(M0)):.2e}")
    assert np.all(dev1 <= b1)
    assert np.all(dev2 <= b2)
    # the bound is no blanket: it stays far below the entries themselves
    assert np.max(b1) <= 1e-9 * np.max(d) and np.max(b2) <= 1e-9 * np.max(np.abs(M0))


def test_one_level_is_the_direct_solve():
    H = level0_cases()["poisson-p2"]
    H1 = Hierarchy(H.ops[:1], [], coarse=True)
    op = H1.ops[0]
    b = lc.rhs(op)
    u, info = H1.pcg(b, np.zeros(op.fixed.size), rtol=1e-10, maxit=5)
    print(f"one level, n = {H1.coarse_factor()[0].size}: {info['iterations']} iterations")
    assert info["converged"] == 1 and info["iterations"] <= 2


# ---- 3. the whole preconditioner as a dense matrix ---------------------------------------------------------------------
def dense_preconditioner(H):
    n = H.ops[-1].fixed.size
    return np.stack([H.precondition(e) for e in np.eye(n)], axis=1)


def abs_preconditioner(H):
    """the recursion of the statement with absolute values: F (|P| M |P|^T + A D^-1) F with the active rows A of the
    rule (all rows without the local rule), and on level 0 |W|^T D^-1 |W| on the free rows"""
    M = None
    for l, op in enumerate(H.ops):
        free = (~op.fixed).astype(np.float64)
        if l == 0:
            rows, d, W = H.coarse_factor()
            D = np.zeros((op.fixed.size, op.fixed.size))
            D[np.ix_(rows, rows)] = np.abs(W).T @ np.diag(1.0 / d) @ np.abs(W)
        else:
            act = H.active(l) if H.local else np.ones(op.fixed.size)
            D = np.diag(act / np.abs(H.diag(l)))
            pcell, npf = H.links[l - 1]
            P = np.kron(np.abs(mc.dense_prolongation(H.ops[l - 1].mesh, op.mesh, pcell, npf, H.p)), np.eye(H.bs))
            D = P @ M @ P.T + D
        M = free[:, None] * D * free[None, :]
    return M


@pytest.mark.parametrize("local", [False, True])
@pytest.mark.parametrize("problem,p", [("poisson", 1), ("poisson", 2), ("elasticity", 1), ("elasticity", 2)])
def test_coarse_preconditioner_is_symmetric_positive_definite(problem, p, local):
    meshes, links = levels()
    v = variants(meshes, links, p, problem)
    H, H0 = v[(local, True)], v[(local, False)]
    assert H.nlevels == 3 and H.ops[-1].fixed.size <= 600 and H.coarse is True and H.local is local
    M = dense_preconditioner(H)
    fixed = H.ops[-1].fixed
    assert np.all(M[fixed] == 0.0) and np.all(M[:, fixed] == 0.0)
    assert not np.array_equal(M, dense_preconditioner(H0))
    # the count of tests/test_multilevel_local_host.py (per level the roundings of one restriction, one prolongation and
    # three single operations, on either of the two entries compared), and for level 0 the two passes of the solve:
    # n0 products and n0 sums each, and the division
    nd = (p + 1) * (p + 2) // 2
    n0 = H.coarse_factor()[0].size
    terms = 2 * (sum(mc.restrict_terms(m, p)[0] + nd + 3 for m in meshes) + 2 * (2 * n0 + 1))
    Mabs = abs_preconditioner(H)
    asym = np.abs(M - M.T)
    print(f"{problem} p={p} local={local}: {fixed.size} rows, {n0} coarse rows, max asymmetry / (2^-53 abs-sum) "
          f"{np.max(asym[Mabs > 0] / (U * Mabs[Mabs > 0])):.2f}, allowed {terms}")
    assert np.all(asym <= terms * U * Mabs)
    lam = np.linalg.eigvalsh(0.5 * (M + M.T)[~fixed][:, ~fixed])
    print(f"eigenvalues of the free block: {lam[0]:.3e} ... {lam[-1]:.3e}")
    assert lam[0] > 0.0


# ---- 4. the switch off ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("local", [False, True])
@pytest.mark.parametrize("problem,p", [("poisson", 2), ("elasticity", 1)])
def test_switch_off_gives_the_bits_of_the_rule_without_it(problem, p, local):
    """coarse=False (the default) against the rule written out here as it stood before the switch"""
    meshes, links = levels()
    H = variants(meshes, links, p, problem)[(local, False)]
    assert H.coarse is False and Hierarchy(H.ops, H.links).coarse is False
    r = np.random.default_rng(8 * p).standard_normal(H.ops[-1].fixed.size)
    L = H.nlevels - 1
    rs = [None] * (L + 1)
    rs[L] = np.where(H.ops[L].fixed, 0.0, r)
    for l in range(L - 1, -1, -1):
        rs[l] = H.restrict(l, rs[l + 1])
    z = np.where(H.ops[0].fixed, 0.0, rs[0] / H.diag(0))
    for l in range(1, L + 1):
        t = H.prolong(l - 1, z)
        z = t + rs[l] / H.diag(l)
        if local:
            z = np.where(H.active(l), z, t)
        z = np.where(H.ops[l].fixed, 0.0, z)
    assert np.array_equal(H.precondition(r).view(np.uint64), z.view(np.uint64))
    assert np.array_equal(Hierarchy(H.ops, H.links, local=local).precondition(r).view(np.uint64), z.view(np.uint64))


# ---- 5. iteration counts on the graded hierarchy from 256 cells ----------------------------------------------------------
@pytest.mark.parametrize("problem,p", [("poisson", 1), ("elasticity", 1), ("poisson", 2)])
def test_coarse_solve_needs_no_more_iterations(problem, p):
    """create_unit_square(8) and 6 graded refinements, rtol 1e-8 from zero.  When the rule was written: full / local
    52 / 40 with the coarse solve against 70 / 71 without (Poisson P_1), 145 / 84 against 151 / 150 (elasticity [P_1]^2),
    57 / 40 against 154 / 183 (Poisson P_2)."""
    meshes, links = graded8()
    assert len(meshes) == 7 and meshes[0].ncells == 256
    v = variants(meshes, links, p, problem)
    op = v[(False, False)].ops[-1]
    b = lc.rhs(op)
    it = {}
    for key, H in v.items():
        _, info = H.pcg(b, np.zeros(op.fixed.size), rtol=1e-8, maxit=2000)
        assert info["converged"] == 1, key
        it[key] = info["iterations"]
    print(f"{problem} p={p}: {op.fixed.size} fine rows, {v[(False, True)].coarse_factor()[0].size} coarse rows; "
          f"full {it[(False, False)]}, local {it[(True, False)]}, full + coarse {it[(False, True)]}, "
          f"local + coarse {it[(True, True)]}")
    assert it[(False, True)] <= it[(False, False)]
    assert it[(True, True)] <= it[(True, False)]
    assert it[(True, True)] <= it[(False, True)]


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals():
    meshes, links = levels()
    H = variants(meshes, links, 1, "poisson")[(False, False)]
    with pytest.raises(ValueError, match="coarse_factor.*coarse=False"):
        H.coarse_factor()
    kappa = pc.kappa_of(meshes[0].ncells)
    free = mc.poisson_op(meshes[0], 1, kappa, facets=np.zeros(0, dtype=np.int32))
    assert not free.fixed.any()
    with pytest.raises(ValueError, match="component 0 of level 0 has no Dirichlet DOF"):
        Hierarchy([free] + H.ops[1:], H.links, coarse=True)
    Hierarchy([free] + H.ops[1:], H.links)   # (without the switch level 0 may be singular: its diagonal is not)
    # a pivot that is not positive
    neg = mc.poisson_op(meshes[0], 1, -kappa)
    with pytest.raises(ValueError, match="singular: pivot 0 "):
        Hierarchy([neg], [], coarse=True).coarse_factor()


def test_pcg_many_uses_the_coarse_solve():
    meshes, links = levels()
    H = variants(meshes, links, 2, "poisson")[(True, True)]
    op = H.ops[-1]
    B = np.random.default_rng(5).standard_normal((2, op.ndofs))
    U0 = np.zeros_like(B)
    X, infos = H.pcg_many(B, U0, rtol=1e-10)
    for c in range(2):
        x, info = H.pcg(B[c], U0[c], rtol=1e-10)
        assert np.array_equal(X[c], x) and infos[c] == info


# ---- 7. the C ABI without a device ---------------------------------------------------------------------------------------
def test_new_entries_are_declared_exported_and_bound():
    from dolfinx_eqlb_amd import cpp
    header = open(os.path.join(ROOT, "include", "eqlb.h")).read()
    L = cpp.lib()
    for name in NEW_ENTRIES:
        assert re.search(r"^int\s+" + name + r"\(", header, flags=re.M), name
        assert name in cpp.EXPORTED_SYMBOLS, name
        assert hasattr(L, name), name
    for name in ("coarse", "set_coarse", "coarse_rows", "coarse_factor", "coarse_factor_raw"):
        assert hasattr(cpp.Multilevel, name), name
    from dolfinx_eqlb_amd import _cpp
    for name in ("coarse", "coarse_rows", "coarse_factor"):
        assert hasattr(_cpp.Multilevel, name), name
    assert "coarse" in _cpp.Multilevel.__init__.__doc__
    tuning = open(os.path.join(ROOT, "dolfinx_eqlb_amd", "csrc", "eqlb_tuning.h")).read()
    assert re.search(r"^#define EQLB_COARSE_MAX_ROWS 4096\b", tuning, flags=re.M)
    makefile = open(os.path.join(ROOT, "dolfinx_eqlb_amd", "csrc", "Makefile")).read()
    assert "eqlb_coarse.hip" in makefile


def test_new_entries_refuse_null_arguments():
    from dolfinx_eqlb_amd import cpp
    L = cpp.lib()
    rows = np.full(4, 7, dtype=np.int32)
    d, W = np.full(4, 7.0), np.full(16, 7.0)
    n = C.c_int64(5)
    fake = C.c_void_p(0x5EED5EED)   # never dereferenced: the refusal comes first
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.eqlb_hierarchy_set_coarse(None, C.c_int32(1), None) == INVALID_ARGUMENT
    assert "eqlb_hierarchy_set_coarse" in L.eqlb_last_error().decode()
    assert L.eqlb_hierarchy_coarse_rows(None, C.byref(n)) == INVALID_ARGUMENT
    assert "eqlb_hierarchy_coarse_rows" in L.eqlb_last_error().decode()
    assert L.eqlb_hierarchy_coarse_rows(fake, None) == INVALID_ARGUMENT
    assert L.eqlb_hierarchy_coarse_factor(None, vp(rows), vp(d), vp(W), C.c_int64(4), C.c_int32(0),
                                          None) == INVALID_ARGUMENT
    assert "eqlb_hierarchy_coarse_factor" in L.eqlb_last_error().decode()
    for args in ((None, vp(d), vp(W)), (vp(rows), None, vp(W)), (vp(rows), vp(d), None)):
        assert L.eqlb_hierarchy_coarse_factor(fake, *args, C.c_int64(4), C.c_int32(0), None) == INVALID_ARGUMENT
    assert np.all(rows == 7) and np.all(d == 7.0) and np.all(W == 7.0) and n.value == 5
