"""Local smoothing of the multilevel preconditioner (lsolver.multilevel.Hierarchy(..., local=True)) as far as it can be
checked without a device: the active sets against the prolongation built as a dense matrix, the preconditioner as a
dense matrix (symmetric within rounding, positive definite on the free rows), uniform refinement (every row active, the
bits of the full sum), the iteration counts on the graded hierarchy of tests/multilevel_local_cases.py, and the new
entries of the C ABI as far as they need no mesh.

The small hierarchy is that of tests/test_multilevel_host.py: create_unit_square(3, shuffle_seed=3, perturb=0.15) with
36 cells, refined at refine_cases.level_marks (parents with 1, 2, 3 and 4 children)."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import multilevel_cases as mc
import multilevel_local_cases as lc
import primal_cases as pc
from dolfinx_eqlb_amd.lsolver.multilevel import Hierarchy
from dolfinx_eqlb_amd.mesh import create_unit_square
from dolfinx_eqlb_amd.mesh import transfer as tr
from refine_cases import level_marks

U = pc.U
INVALID_ARGUMENT = -1
NEW_ENTRIES = ("eqlb_hierarchy_set_local", "eqlb_hierarchy_active", "eqlb_hierarchy_active_count")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def levels():
    """three levels: 36 cells, refined at level_marks(., 1), then at level_marks(., 2)"""
    if "levels" not in _CACHE:
        base = create_unit_square(3, shuffle_seed=3, perturb=0.15)
        _CACHE["levels"] = mc.levels_host(base, [lambda n: level_marks(n, 1), lambda n: level_marks(n, 2)])
    return _CACHE["levels"]


def local_hierarchy(meshes, links, p, problem):
    """(the full statement, the local one on the same operators)"""
    H, _ = mc.hierarchy(meshes, links, p, problem)
    return H, Hierarchy(H.ops, H.links, local=True)


# ---- 1. the active sets ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_active_rows_against_the_dense_prolongation(p):
    """an inactive row is a unit row of P (its basis function is the one of the level below); every row that is no unit
    row is active; and the set is the union of the dofmap rows of the children of bisected cells, entry by entry"""
    meshes, links = levels()
    pcell, npf = links[0]
    assert sorted(set(np.bincount(pcell, minlength=meshes[0].ncells))) == [1, 2, 3, 4]
    _, HL = local_hierarchy(meshes[:2], links[:1], p, "poisson")
    act = HL.active(1)
    P = mc.dense_prolongation(meshes[0], meshes[1], pcell, npf, p)
    assert act.dtype == bool and act.shape == (P.shape[0],)
    unit = (np.sum(P == 1.0, axis=1) == 1) & (np.sum(P != 0.0, axis=1) == 1)
    print(f"p={p}: {P.shape[0]} rows, {int(act.sum())} active, {int(unit.sum())} unit rows of P")
    assert 0 < act.sum() < act.size
    assert np.all(unit[~act])
    assert np.all(act[~unit])
    cell_dofs, ndofs = tr.lagrange_dofmap(meshes[1], p)
    kids = np.bincount(pcell, minlength=meshes[0].ncells)
    ref = np.zeros(ndofs, dtype=bool)
    for c2 in range(meshes[1].ncells):
        if kids[pcell[c2]] > 1:
            ref[cell_dofs[c2]] = True
    assert np.array_equal(act, ref)
    assert np.all(HL.active(0)) and HL.active(0).size == HL.ops[0].fixed.size
    # two rows per DOF on a vector space
    _, HE = local_hierarchy(meshes[:2], links[:1], p, "elasticity")
    assert np.array_equal(HE.active(1), np.repeat(ref, 2))


def test_active_refusals():
    meshes, links = levels()
    H, HL = local_hierarchy(meshes, links, 1, "poisson")
    assert H.local is False and HL.local is True
    with pytest.raises(ValueError, match="local=False"):
        H.active(1)
    for level in (-1, 3):
        with pytest.raises(ValueError, match=f"level = {level} outside 0 ... 2"):
            HL.active(level)


def test_every_fine_row_is_reached():
    """P_1 on the graded hierarchy: the nodes keep their numbers from level to level and new ones are appended, so node
    n appears on the first level with more than n nodes - and is active there (level 0: every row)"""
    meshes, links = lc.graded_levels_host(8)
    _, HL = local_hierarchy(meshes, links, 1, "poisson")
    nn = np.array([m.nnodes for m in meshes])
    first = np.searchsorted(nn, np.arange(nn[-1]), side="right")   # the level on which node n appears
    for l in range(HL.nlevels):
        assert np.all(HL.active(l)[first[:nn[l]] == l]), l
    total, active = sum(o.fixed.size for o in HL.ops), sum(int(HL.active(l).sum()) for l in range(HL.nlevels))
    print(f"{HL.nlevels} levels, {total} rows over all levels, {active} active")
    assert active < total


# ---- 2. the preconditioner as a dense matrix ---------------------------------------------------------------------------
def dense_preconditioner(H):
    n = H.ops[-1].fixed.size
    return np.stack([H.precondition(e) for e in np.eye(n)], axis=1)


def abs_preconditioner(H):
    """the recursion of the local statement with absolute values: F (|P| M |P|^T + A D^-1) F, A the active rows"""
    M = None
    for l, op in enumerate(H.ops):
        free = (~op.fixed).astype(np.float64)
        D = np.diag(H.active(l) / np.abs(H.diag(l)))
        if M is not None:
            pcell, npf = H.links[l - 1]
            P = np.kron(np.abs(mc.dense_prolongation(H.ops[l - 1].mesh, op.mesh, pcell, npf, H.p)), np.eye(H.bs))
            D = P @ M @ P.T + D
        M = free[:, None] * D * free[None, :]
    return M


@pytest.mark.parametrize("problem,p", [("poisson", 1), ("poisson", 2), ("elasticity", 1), ("elasticity", 2)])
def test_local_preconditioner_is_symmetric_positive_definite(problem, p):
    meshes, links = levels()
    H, HL = local_hierarchy(meshes, links, p, problem)
    assert HL.nlevels == 3 and HL.ops[-1].fixed.size <= 600 and HL.bs == (1 if problem == "poisson" else 2)
    assert all(0 < HL.active(l).sum() < HL.active(l).size for l in (1, 2))
    M = dense_preconditioner(HL)
    fixed = HL.ops[-1].fixed
    assert np.all(M[fixed] == 0.0) and np.all(M[:, fixed] == 0.0)
    assert not np.array_equal(M, dense_preconditioner(H))
    # the count of tests/test_multilevel_host.py: per level the roundings of one restriction, one prolongation (nd_p) and
    # three single operations, on either of the two entries compared
    nd = (p + 1) * (p + 2) // 2
    terms = 2 * sum(mc.restrict_terms(m, p)[0] + nd + 3 for m in meshes)
    Mabs = abs_preconditioner(HL)
    asym = np.abs(M - M.T)
    print(f"{problem} p={p}: {fixed.size} rows, max asymmetry / (2^-53 abs-sum) "
          f"{np.max(asym[Mabs > 0] / (U * Mabs[Mabs > 0])):.2f}, allowed {terms}")
    assert np.all(asym <= terms * U * Mabs)
    lam = np.linalg.eigvalsh(0.5 * (M + M.T)[~fixed][:, ~fixed])
    print(f"eigenvalues of the free block: {lam[0]:.3e} ... {lam[-1]:.3e}")
    assert lam[0] > 0.0


def test_an_inactive_row_takes_the_prolonged_value_as_it_is():
    """no addition on an inactive free row: it has the bits of the prolonged vector, zeros with their sign included, for
    a random r and for r = -0.0 on the free rows"""
    meshes, links = levels()
    _, HL = local_hierarchy(meshes[:2], links[:1], 1, "poisson")
    lo, op = HL.ops
    inactive = ~HL.active(1) & ~op.fixed
    assert inactive.any()
    for r in (np.random.default_rng(6).standard_normal(op.ndofs), np.where(op.fixed, 0.0, -0.0)):
        z = HL.precondition(r)
        r0 = HL.restrict(0, np.where(op.fixed, 0.0, r))
        t = HL.prolong(0, np.where(lo.fixed, 0.0, r0 / HL.diag(0)))
        assert np.array_equal(z[inactive].view(np.uint64), t[inactive].view(np.uint64))
        assert np.all(z[op.fixed] == 0.0) and not np.any(np.signbit(z[op.fixed]))
    assert np.all(t[inactive] == 0.0)   # (the last r)


# ---- 3. uniform refinement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem,p", [("poisson", 1), ("poisson", 3), ("elasticity", 2)])
def test_uniform_refinement_is_the_full_sum(problem, p):
    base = create_unit_square(3, shuffle_seed=3, perturb=0.15)
    meshes, links = mc.levels_host(base, [mc.all_cells] * 2)
    H, HL = local_hierarchy(meshes, links, p, problem)
    for l in range(3):
        assert np.all(HL.active(l)) and HL.active(l).size == HL.ops[l].fixed.size
    r = np.random.default_rng(3 * p).standard_normal(H.ops[-1].fixed.size)
    assert np.array_equal(HL.precondition(r).view(np.uint64), H.precondition(r).view(np.uint64))


# ---- 4. iteration counts on the graded hierarchy --------------------------------------------------------------------------
def counts(problem, p, nref=8):
    meshes, links = lc.graded_levels_host(nref)
    assert len(meshes) == 9 and [meshes[0].ncells, meshes[-1].ncells] == [64, 1817]
    H, HL = local_hierarchy(meshes, links, p, problem)
    op = H.ops[-1]
    b = lc.rhs(op)
    out = []
    for h in (H, HL):
        _, info = h.pcg(b, np.zeros(op.fixed.size), rtol=1e-8, maxit=2000)
        assert info["converged"] == 1
        out.append(info["iterations"])
    print(f"{problem} p={p}: {H.nlevels} levels, {op.fixed.size} fine rows, full BPX {out[0]} iterations, local {out[1]}")
    return out


@pytest.mark.parametrize("problem", ["poisson", "elasticity"])
def test_local_smoothing_needs_no_more_iterations_at_p1(problem):
    """9 levels, 64 -> 1 817 cells: 51 -> 37 for Poisson, 151 -> 89 for elasticity when this was written (12
    refinements, 8 509 cells: 64 -> 41 for Poisson).  The gain needs a coarse level 0: from create_unit_square(16) the
    same marking gives 124 -> 150 on 9 levels (the section on local smoothing)."""
    full, local = counts(problem, 1)
    assert local <= full


def test_counts_at_p2_are_reported():
    """no claim at p >= 2: both converge, the counts are printed (80 and 83 when this was written)"""
    counts("poisson", 2)


def test_pcg_many_uses_the_local_preconditioner():
    meshes, links = levels()
    _, HL = local_hierarchy(meshes, links, 2, "poisson")
    op = HL.ops[-1]
    B = np.random.default_rng(5).standard_normal((2, op.ndofs))
    U0 = np.zeros_like(B)
    X, infos = HL.pcg_many(B, U0, rtol=1e-10)
    for c in range(2):
        x, info = HL.pcg(B[c], U0[c], rtol=1e-10)
        assert np.array_equal(X[c], x) and infos[c] == info


# ---- 5. the C ABI without a device ------------------------------------------------------------------------------------------
def test_new_entries_are_declared_exported_and_bound():
    from dolfinx_eqlb_amd import cpp
    header = open(os.path.join(ROOT, "include", "eqlb.h")).read()
    L = cpp.lib()
    for name in NEW_ENTRIES:
        assert re.search(r"^int\s+" + name + r"\(", header, flags=re.M), name
        assert name in cpp.EXPORTED_SYMBOLS, name
        assert hasattr(L, name), name
    for name in ("local", "set_local", "active", "active_raw", "active_count"):
        assert hasattr(cpp.Multilevel, name), name
    from dolfinx_eqlb_amd import _cpp
    for name in ("local", "active", "active_count"):
        assert hasattr(_cpp.Multilevel, name), name
    assert "local" in _cpp.Multilevel.__init__.__doc__


def test_new_entries_refuse_null_arguments():
    from dolfinx_eqlb_amd import cpp
    L = cpp.lib()
    out = np.full(4, 7, dtype=np.uint8)
    n = C.c_int64(5)
    fake = C.c_void_p(0x5EED5EED)   # never dereferenced: the refusal comes first
    assert L.eqlb_hierarchy_set_local(None, C.c_int32(1), None) == INVALID_ARGUMENT
    assert "eqlb_hierarchy_set_local" in L.eqlb_last_error().decode()
    assert L.eqlb_hierarchy_active(None, C.c_int32(0), out.ctypes.data_as(C.c_void_p), C.c_int64(4), C.c_int32(0),
                                   None) == INVALID_ARGUMENT
    assert "eqlb_hierarchy_active" in L.eqlb_last_error().decode()
    assert L.eqlb_hierarchy_active(fake, C.c_int32(0), None, C.c_int64(4), C.c_int32(0), None) == INVALID_ARGUMENT
    assert L.eqlb_hierarchy_active_count(None, C.c_int32(0), C.byref(n)) == INVALID_ARGUMENT
    assert "eqlb_hierarchy_active_count" in L.eqlb_last_error().decode()
    assert L.eqlb_hierarchy_active_count(fake, C.c_int32(0), None) == INVALID_ARGUMENT
    assert np.all(out == 7) and n.value == 5
