"""The exact solve on level 0 of the multilevel preconditioner on the device (cpp.Multilevel(..., coarse=True),
eqlb_hierarchy_set_coarse / _coarse_rows / _coarse_factor, csrc/eqlb_coarse.hip) against its numpy statement
(lsolver.multilevel.Hierarchy(..., coarse=True)): the factor bit for bit at the sizes where the kernels change their
path, the preconditioner bit for bit in both memory spaces and for several columns, the solves, the refusals, the
switch and the snapshot, a caller's stream, and the pybind carrier against the ctypes route.

The hierarchies: the three levels of tests/test_multilevel_coarse_host.py (36 cells, refined at refine_cases.level_marks)
and create_unit_square(8) with six graded refinements, both refined on the device with the plans kept."""

import os
import re

import numpy as np
import pytest

import multilevel_cases as mc
import multilevel_local_cases as lc
import primal_mesh_cases as pm
import test_gpu_primal_meshes as gm
from dolfinx_eqlb_amd.lsolver import primal
from dolfinx_eqlb_amd.lsolver.multilevel import Hierarchy
from dolfinx_eqlb_amd.mesh import create_unit_square
from refine_cases import level_marks
from test_gpu_multilevel import allowance
from test_gpu_primal_elasticity import check_solution as check_elasticity
from test_gpu_primal_many import compare
from test_gpu_primal_solve import bits
from test_gpu_primal_solve import check_solution as check_poisson

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def tuning(name):
    text = open(os.path.join(ROOT, "dolfinx_eqlb_amd", "csrc", "eqlb_tuning.h")).read()
    return int(re.search(r"^#define " + name + r" (\d+)\b", text, flags=re.M).group(1))


# the sizes of csrc/eqlb_coarse.hip: the columns of a block step of the factor (also the tile of the transposition), and
# the tile of the trailing updates (also the workgroup of the panel kernels and of the two kernels of an application)
BLOCK, TILE, MAX_ROWS = tuning("EQLB_COARSE_BLOCK"), tuning("EQLB_COARSE_TILE"), tuning("EQLB_COARSE_MAX_ROWS")
TARGETS = sorted({1, 2} | {m * s + o for s in (BLOCK, TILE) for m in (1, 2) for o in (-1, 0, 1)})
CONFIGS = [("poisson", 1), ("poisson", 2), ("poisson", 3), ("poisson", 4), ("elasticity", 1), ("elasticity", 2)]


def same_factor(ml, H):
    rows, d, W = H.coarse_factor()
    assert ml.coarse_rows == rows.size
    grows, gd, gW = ml.coarse_factor()
    assert grows.dtype == np.int32 and np.array_equal(grows, rows)
    assert gW.shape == (rows.size, rows.size)
    assert np.array_equal(bits(gd), bits(d))
    assert np.array_equal(bits(gW), bits(W))
    assert np.all(np.diag(gW) == 1.0) and np.all(np.triu(gW, 1) == 0.0)


# ---- 1. the factor, bit for bit ------------------------------------------------------------------------------------------
def free_rows(op, lists):
    op.set_dirichlet(*lists)
    return int((~op.fixed).sum())


def steering_meshes():
    """the one-cell and the two-cell mesh, then create_rectangle(nx, ny) for 1 <= nx <= ny <= 8, smallest first, then
    create_disk(k, rings) for 3 <= k <= 24 cells round the centre and 1 ... 3 rings.  The boundary facets are numbered
    along the boundary, so a prefix of m of them fixes p m + 1 DOFs per row and the count of free rows keeps its
    residue modulo p on one mesh: the residues come from the variety of the meshes"""
    if "steer" not in _CACHE:
        from dolfinx_eqlb_amd.mesh import create_disk, create_rectangle
        shapes = sorted(((nx, ny) for ny in range(1, 9) for nx in range(1, ny + 1)), key=lambda s: (s[0] * s[1], s))
        _CACHE["steer"] = ([pm.mesh_of("triangle"), pm.mesh_of("right1")] + [create_rectangle(nx, ny) for nx, ny in shapes]
                           + [create_disk(k, rings) for rings in (1, 2, 3) for k in range(3, 25)])
    return _CACHE["steer"]


def steer(problem, p):
    """{free rows: (mesh, coefficient, arguments of set_dirichlet)} for the TARGETS that can be met: Dirichlet conditions
    on a prefix of mesh.boundary_facets() - for elasticity a prefix for each of the two rows - on the first of
    steering_meshes() on which the count of free rows is the target exactly.  Every prefix of every mesh is counted on
    the statement until all targets are met (the one-cell and two-cell meshes carry Poisson cases only)."""
    if ("table", problem, p) in _CACHE:
        return _CACHE["table", problem, p]
    table = {}
    for index, mesh in enumerate(steering_meshes()):
        if len(table) == len(TARGETS):
            break
        if problem == "elasticity" and index < 2:
            continue
        bf = mesh.boundary_facets().astype(np.int32)
        if problem == "poisson":
            coeff = pm.pc.kappa_of(mesh.ncells)
            op = primal.PoissonOperator(mesh, p, coeff)
            for m in range(1, bf.size + 1):
                n = free_rows(op, (bf[:m],))
                if n in TARGETS and n not in table:
                    table[n] = (mesh, coeff, (bf[:m],))
        else:
            coeff = pm.ec.pi1_of(mesh.ncells)
            op = primal.ElasticityOperator(mesh, p, cell_pi1=coeff)
            per_row = [free_rows(op, (bf[:m], bf[:m])) // 2 for m in range(1, bf.size + 1)]   # per_row[m - 1]
            for m0 in range(1, bf.size + 1):
                for m1 in range(1, bf.size + 1):
                    n = per_row[m0 - 1] + per_row[m1 - 1]
                    if n in TARGETS and n not in table:
                        table[n] = (mesh, coeff, (bf[:m0], bf[:m1]))
    _CACHE["table", problem, p] = table
    return table


def can_be_met(problem, p, target):
    """Whether a prefix of the boundary facets can leave `target` free rows.  On a simply connected mesh of V nodes, E
    edges and C cells, E = V + C - 1.  A P_p cell has (p - 1)(p - 2) / 2 interior DOFs that no facet fixes, and a prefix
    that fixes all but the interior of one or two cells leaves too few or too many rows for 1 and 2 at p >= 3; they are
    required of Poisson at P_1 and P_2 (the vector problem doubles the rows).  P_3 has 3 V + 3 C - 2 DOFs, a prefix of m
    facets fixes 3 m + 1 of them and the whole boundary 3 m: the free count is 0 or 1 modulo 3.  P_4 has 4 V + 6 C - 3
    DOFs, a prefix fixes 4 m + 1: the free count is even unless the whole boundary is fixed, so odd targets are taken
    where a mesh happens to meet them.  Every other target is required."""
    if target < BLOCK - 1:
        return problem == "poisson" and p <= 2
    if p == 3:
        return target % 3 != 2
    if p == 4:
        return target % 2 == 0
    return True


@pytest.mark.parametrize("problem,p", CONFIGS)
def test_factor_bit_for_bit_at_the_block_and_tile_boundaries(problem, p):
    """n = 1, 2 and one below / at / one above the first and second multiple of the block and of the tile, wherever a
    prefix of the boundary facets can meet the count (can_be_met: which targets that excludes, and why)."""
    from dolfinx_eqlb_amd import cpp
    assert (BLOCK, TILE) == (32, 64) and TARGETS == [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129]
    met = []
    table = steer(problem, p)
    for target in TARGETS:
        if target not in table:
            assert not can_be_met(problem, p, target), target
            continue
        mesh, coeff, args = table[target]
        op = pm.statement(problem, mesh, p, "all", coeff)[0]
        op.set_dirichlet(*args)
        assert int((~op.fixed).sum()) == target
        H = Hierarchy([op], [], coarse=True)
        h = gm.make_handle(problem, cpp.DeviceMesh(mesh), p, coeff, args)
        ml = cpp.Multilevel([h], [], coarse=True)
        assert ml.coarse is True and ml.coarse_rows == target
        same_factor(ml, H)
        r = np.random.default_rng(target).standard_normal(op.fixed.size)
        assert np.array_equal(bits(ml.precondition(r)), bits(H.precondition(r)))
        ml.close()
        met.append(target)
    print(f"{problem} p={p}: targets met {met}")


def test_every_target_is_met_at_the_low_degrees_of_both_problems():
    for target in TARGETS:
        configs = [c for c in CONFIGS if target in steer(*c)]
        assert len(configs) >= 3, (target, configs)
        if target >= BLOCK - 1:
            assert {("poisson", 1), ("poisson", 2), ("elasticity", 1), ("elasticity", 2)} <= set(configs), target


def test_factor_bit_for_bit_with_the_whole_boundary_fixed():
    """create_unit_square(8) at P_2: n = 481, 16 block steps with a last block of one column"""
    c = case("poisson", "graded8", 2)
    assert c["HC"][False].coarse_factor()[0].size == 481 and 481 % BLOCK == 1
    same_factor(c["ml"], c["HC"][False])


@pytest.mark.parametrize("name,p", [("triangle", 1), ("right1", 1), ("triangle", 2)])
def test_no_free_row(name, p):
    """level 0 without a free row: nothing is factored, z_0 = 0, and the bits are the statement's - as one level and
    below a refined level"""
    from dolfinx_eqlb_amd import cpp
    dm = cpp.DeviceMesh(pm.mesh_of(name))
    ref = dm.refine(mc.all_cells(dm.mesh.ncells), keep_plan=True)
    ops, hs = [], []
    for d in (dm, ref.dmesh):
        op, k, args = pm.statement("poisson", d.mesh, p, "all")
        ops.append(op)
        hs.append(gm.make_handle("poisson", d, p, k, args))
    assert not (~ops[0].fixed).any()
    for nlevels in (1, 2):
        H = Hierarchy(ops[:nlevels], [ref][:nlevels - 1], coarse=True)
        ml = cpp.Multilevel(hs[:nlevels], [ref][:nlevels - 1], coarse=True)
        assert ml.coarse_rows == 0
        rows, d, W = ml.coarse_factor()
        assert rows.size == 0 and d.size == 0 and W.shape == (0, 0)
        r = np.random.default_rng(3).standard_normal(ops[nlevels - 1].fixed.size)
        z = ml.precondition(r)
        assert np.array_equal(bits(z), bits(H.precondition(r)))
        if nlevels == 1:
            assert np.all(z == 0.0) and not np.any(np.signbit(z))
        ml.close()


# ---- the hierarchies -------------------------------------------------------------------------------------------------------
def device_levels(name):
    """(DeviceMesh per level, Refinement per link), refined on the device with the plans kept"""
    if ("levels", name) not in _CACHE:
        from dolfinx_eqlb_amd import cpp
        if name == "three":
            dms, refs = [cpp.DeviceMesh(create_unit_square(3, shuffle_seed=3, perturb=0.15))], []
            for step in (1, 2):
                refs.append(dms[-1].refine(level_marks(dms[-1].mesh.ncells, step), keep_plan=True))
                dms.append(refs[-1].dmesh)
            assert dms[0].mesh.ncells == 36
        else:
            assert name == "graded8"
            dms, refs = [cpp.DeviceMesh(create_unit_square(8))], []
            for _ in range(6):
                refs.append(dms[-1].refine(lc.graded_marks(dms[-1].mesh), keep_plan=True))
                dms.append(refs[-1].dmesh)
            assert dms[0].mesh.ncells == 256 and len(dms) == 7
        _CACHE["levels", name] = (dms, refs)
    return _CACHE["levels", name]


def case(problem, name, p, nlevels=None):
    """ops and handles of one (problem, hierarchy, p), Dirichlet all around; HC[local]: the statements with the coarse
    solve (one factor, shared); ml: a Multilevel with coarse=True whose `local` the tests switch"""
    key = (problem, name, p, nlevels)
    if key not in _CACHE:
        from dolfinx_eqlb_amd import cpp
        dms, refs = device_levels(name)
        if nlevels is not None:
            dms, refs = dms[:nlevels], refs[:nlevels - 1]
        meshes = [d.mesh for d in dms]
        links = [(r.parent_cell, r.node_parent_facet) for r in refs]
        coeff = mc.coefficients(meshes, links, pm.pc.kappa_of if problem == "poisson" else pm.ec.pi1_of)
        ops, hs = [], []
        for dm, m, k in zip(dms, meshes, coeff):
            op, _, args = pm.statement(problem, m, p, "all", k)
            ops.append(op)
            hs.append(gm.make_handle(problem, dm, p, k, args))
        HC = {False: Hierarchy(ops, refs, coarse=True), True: Hierarchy(ops, refs, local=True, coarse=True)}
        HC[True]._factor = HC[False].coarse_factor()   # (the same operators: the same factor)
        c = dict(ops=ops, hs=hs, refs=refs, meshes=meshes, coeff=coeff, HC=HC, H0=Hierarchy(ops, refs),
                 ml=cpp.Multilevel(hs, refs, coarse=True))
        assert c["ml"].coarse is True and c["ml"].local is False
        _CACHE[key] = c
    return _CACHE[key]


# ---- 2. the preconditioner, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three", "graded8"])
@pytest.mark.parametrize("problem,p", CONFIGS)
def test_coarse_precondition_bit_for_bit(problem, p, name):
    """full and local rule, host and device memory; a second call gives the same bits.  (graded8 at P_4 has 1 985 coarse
    rows: the numpy factor of the statement takes its seconds once.)"""
    import torch
    c = case(problem, name, p)
    ml, HC = c["ml"], c["HC"]
    n = c["ops"][-1].fixed.size
    r = np.random.default_rng(pm.seed_of("coarse", problem, name, p)).standard_normal(n)
    same_factor(ml, HC[False])
    dev = torch.device("cuda:0")
    for local in (False, True):
        ml.local = local
        want = HC[local].precondition(r)
        for call in range(2):
            z = ml.precondition(r)
            assert np.array_equal(bits(z), bits(want)), (local, call)
        assert np.all(z[c["ops"][-1].fixed] == 0.0)
        d_r = torch.from_numpy(r).to(dev)
        d_z = torch.full_like(d_r, float("nan"))
        torch.cuda.synchronize()
        ml.precondition_raw(d_r.data_ptr(), d_z.data_ptr())
        assert np.array_equal(bits(d_z.cpu().numpy()), bits(want))
        assert np.array_equal(bits(d_r.cpu().numpy()), bits(r))   # the input is not touched
    ml.local = False
    assert not np.array_equal(bits(want), bits(c["H0"].precondition(r)))   # the diagonal of level 0 would show


@pytest.mark.parametrize("problem,p", CONFIGS)
def test_one_level_bit_for_bit(problem, p):
    """one level: the direct solve as a preconditioner, on the caller's vectors"""
    c = case(problem, "three", p, nlevels=1)
    ml, H = c["ml"], c["HC"][False]
    same_factor(ml, H)
    r = np.random.default_rng(11 * p).standard_normal(c["ops"][0].fixed.size)
    z = ml.precondition(r)
    assert np.array_equal(bits(z), bits(H.precondition(r)))
    b = lc.rhs(c["ops"][0])
    u, info = ml.solve(b, np.zeros(b.size), rtol=1e-10, maxit=10)
    assert info["converged"] == 1 and info["iterations"] <= 2


# ---- 3. several columns ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrhs", [1, 3, 5])
@pytest.mark.parametrize("name,p", [("three", 1), ("graded8", 2), ("three", 4)])
def test_coarse_precondition_many(name, p, nrhs):
    """column c has the bits of the single call (5: a second group of four columns); a NaN right-hand side in one
    column leaves the others alone"""
    c = case("poisson", name, p)
    ml, H = c["ml"], c["HC"][True]
    ml.local = True
    fixed = c["ops"][-1].fixed
    V = np.random.default_rng(pm.seed_of("coarse-many", name, p, nrhs)).standard_normal((nrhs, fixed.size))
    single = np.stack([ml.precondition(v) for v in V])
    assert np.array_equal(bits(single[0]), bits(H.precondition(V[0])))
    assert np.array_equal(bits(ml.precondition_many(V)), bits(single))
    bad = nrhs // 2
    Vn = V.copy()
    Vn[bad, np.nonzero(~fixed)[0][7]] = np.nan
    Z = ml.precondition_many(Vn)
    assert np.isnan(Z[bad]).any()
    others = [k for k in range(nrhs) if k != bad]
    assert np.array_equal(bits(Z[others]), bits(single[others]))
    ml.local = False


@pytest.mark.parametrize("nrhs", [1, 3, 5])
def test_coarse_solve_many(nrhs):
    """bits and info of the single solves, which converge; the columns stop at different iterations"""
    c = case("poisson", "graded8", 2)
    ml, op = c["ml"], c["ops"][-1]
    ml.local = True
    rng = np.random.default_rng(pm.seed_of("coarse-solve-many", nrhs))
    B = rng.standard_normal((nrhs, op.ndofs))
    B[nrhs // 2] *= 1e-3
    U0 = np.where(op.fixed, rng.standard_normal((nrhs, op.ndofs)), 0.0)
    infos = compare(ml.solve_many, ml.solve, B, U0, rtol=1e-8, maxit=2000)
    assert all(i["converged"] == 1 for i in infos)
    ml.local = False


# ---- 4. the solves -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("local", [False, True])
@pytest.mark.parametrize("problem,name,p", [("poisson", "graded8", 1), ("elasticity", "graded8", 1),
                                            ("poisson", "three", 3), ("elasticity", "three", 2)])
def test_coarse_solve(problem, name, p, local):
    """rtol 1e-8 from zero: the bounds of check_solution against a direct solve, the count within the allowance of the
    statement's, two solves with the same bits"""
    c = case(problem, name, p)
    ml, H, op = c["ml"], c["HC"][local], c["ops"][-1]
    ml.local = local
    n = op.fixed.size
    b, u0 = lc.rhs(op), np.zeros(n)
    u, info = ml.solve(b, u0, rtol=1e-8, maxit=2000)
    check = check_poisson if problem == "poisson" else check_elasticity
    check(op, pm.assembled(problem, c["meshes"][-1], p, c["coeff"][-1]), b, u0, u, info, 1e-8)
    _, si = H.pcg(b, u0, rtol=1e-8, maxit=2000)
    print(f"{problem} {name} p={p} local={local}: {info['iterations']} iterations, statement {si['iterations']}")
    assert si["converged"] == 1 and abs(si["iterations"] - info["iterations"]) <= allowance(info["iterations"])
    u2, info2 = ml.solve(b, u0, rtol=1e-8, maxit=2000)
    assert np.array_equal(bits(u), bits(u2)) and info == info2
    ml.local = False


def test_local_with_the_coarse_solve_needs_no_more_iterations_on_the_device():
    """create_unit_square(8), six graded refinements, P_1: local + coarse against local on the same handles (40 against
    71 by the statement)"""
    from dolfinx_eqlb_amd import cpp
    c = case("poisson", "graded8", 1)
    op = c["ops"][-1]
    b, u0 = lc.rhs(op), np.zeros(op.fixed.size)
    ml = cpp.Multilevel(c["hs"], c["refs"], local=True)
    _, li = ml.solve(b, u0, rtol=1e-8, maxit=2000)
    ml.coarse = True
    _, ci = ml.solve(b, u0, rtol=1e-8, maxit=2000)
    ml.close()
    print(f"poisson p=1: local {li['iterations']} iterations, local + coarse {ci['iterations']}")
    assert li["converged"] == 1 and ci["converged"] == 1 and ci["iterations"] <= li["iterations"]


def test_large_coarse_level():
    """create_unit_square(16) at P_2 as one level: n = 1 985, 63 block steps and 31 x 31 tiles.  The preconditioner is
    the inverse up to rounding: the CG converges in at most 2 iterations and the true residual (the statement's) is
    under the tolerance"""
    from dolfinx_eqlb_amd import cpp
    mesh = create_unit_square(16)
    op, k, args = pm.statement("poisson", mesh, 2, "all")
    h = gm.make_handle("poisson", cpp.DeviceMesh(mesh), 2, k, args)
    ml = cpp.Multilevel([h], [], coarse=True)
    assert ml.coarse_rows == 1985 == int((~op.fixed).sum())
    b, u0 = lc.rhs(op), np.zeros(op.fixed.size)
    u, info = ml.solve(b, u0, rtol=1e-8, maxit=10)
    r = op.residual(b, u)
    rn = np.sqrt(np.sum(r * r))
    print(f"n = 1985: {info['iterations']} iterations, residual {rn:.3e}, tolerance {1e-8 * info['nb']:.3e}")
    assert info["converged"] == 1 and info["iterations"] <= 2
    assert rn <= 1e-8 * info["nb"] * (1.0 + op.ndofs * pm.pc.U)
    rows, d, W = ml.coarse_factor()
    assert np.array_equal(rows, np.nonzero(~op.fixed)[0]) and np.all(d > 0.0)
    assert np.all(np.diag(W) == 1.0) and np.all(np.triu(W, 1) == 0.0)
    ml.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    from dolfinx_eqlb_amd import cpp
    c = case("poisson", "three", 2)
    ml = cpp.Multilevel(c["hs"], c["refs"])
    assert ml.coarse is False
    out = (np.full(4, 7, dtype=np.int32), np.full(4, 7.0), np.full(16, 7.0))
    with pytest.raises(RuntimeError, match="eqlb_hierarchy_coarse_factor.*eqlb_hierarchy_set_coarse"):
        ml.coarse_factor_raw(out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, 4, cpp.MEM_HOST)
    assert np.all(out[0] == 7) and np.all(out[1] == 7.0) and np.all(out[2] == 7.0)
    with pytest.raises(RuntimeError, match="eqlb_hierarchy_coarse_rows.*eqlb_hierarchy_set_coarse"):
        ml.coarse_rows
    for value in (2, -1):
        with pytest.raises(RuntimeError, match=f"eqlb_hierarchy_set_coarse: coarse = {value} is not 0 or 1"):
            ml.set_coarse(value)
        assert ml.coarse is False
    ml.coarse = True
    n = ml.coarse_rows
    rows, d, W = np.full(n, 7, dtype=np.int32), np.full(n, 7.0), np.full(n * n, 7.0)
    with pytest.raises(RuntimeError, match="eqlb_hierarchy_coarse_factor: capacity"):
        ml.coarse_factor_raw(rows.ctypes.data, d.ctypes.data, W.ctypes.data, n - 1, cpp.MEM_HOST)
    with pytest.raises(RuntimeError, match="unknown memory space"):
        ml.coarse_factor_raw(rows.ctypes.data, d.ctypes.data, W.ctypes.data, n, 5)
    assert np.all(rows == 7) and np.all(d == 7.0) and np.all(W == 7.0)
    ml.close()


def test_more_rows_than_the_cap_are_refused():
    """create_unit_square(46) at P_1: 4 141 free rows"""
    from dolfinx_eqlb_amd import cpp
    mesh = create_unit_square(46)
    h = cpp.PrimalPoisson(cpp.DeviceMesh(mesh), 1)
    h.set_dirichlet(mesh.boundary_facets())
    ml = cpp.Multilevel([h], [])
    r = np.ones(h.ndofs)
    before = ml.precondition(r)
    with pytest.raises(RuntimeError, match=f"eqlb_hierarchy_set_coarse.*4141 free rows.*{MAX_ROWS}") as err:
        ml.set_coarse(True)
    assert cpp.lib().eqlb_hierarchy_set_coarse(ml._h, 1, None) == -3   # EQLB_ERR_UNSUPPORTED
    assert "4141" in str(err.value) and ml.coarse is False
    assert np.array_equal(bits(ml.precondition(r)), bits(before))   # the handle goes on as before
    ml.close()


def test_a_level_0_without_a_dirichlet_dof_is_refused():
    from dolfinx_eqlb_amd import cpp
    c = case("elasticity", "three", 1)
    dms = device_levels("three")[0]
    lists = pm.elasticity_lists(dms[0].mesh, "all")
    h0 = cpp.PrimalElasticity(dms[0], 1, cell_pi1=c["coeff"][0])
    h0.set_dirichlet(lists[0], np.zeros(0, dtype=np.int32))
    ml = cpp.Multilevel([h0] + c["hs"][1:], c["refs"])
    with pytest.raises(RuntimeError, match="eqlb_hierarchy_set_coarse: singular: component 1 of level 0 has no Dirichlet"):
        ml.coarse = True
    assert cpp.lib().eqlb_hierarchy_set_coarse(ml._h, 1, None) == -1
    assert ml.coarse is False
    with pytest.raises(RuntimeError, match="component 1 of level 0"):
        cpp.Multilevel([h0] + c["hs"][1:], c["refs"], coarse=True)
    ml.close()


def test_a_pivot_that_is_not_positive_is_refused():
    """a negative coefficient on level 0: the first pivot is negative; the switch stays off and the handle goes on as
    before"""
    from dolfinx_eqlb_amd import cpp
    c = case("poisson", "three", 2)
    dms = device_levels("three")[0]
    args = pm.statement("poisson", dms[0].mesh, 2, "all")[2]
    h0 = gm.make_handle("poisson", dms[0], 2, -c["coeff"][0], args)
    ml = cpp.Multilevel([h0] + c["hs"][1:], c["refs"])
    r = np.random.default_rng(2).standard_normal(c["ops"][-1].fixed.size)
    before = ml.precondition(r)
    rows = np.nonzero(~c["ops"][0].fixed)[0]
    with pytest.raises(RuntimeError, match=f"eqlb_hierarchy_set_coarse: singular: pivot 0 \\(row {rows[0]} of level 0\\)"):
        ml.set_coarse(True)
    assert cpp.lib().eqlb_hierarchy_set_coarse(ml._h, 1, None) == -6   # EQLB_ERR_SINGULAR
    assert ml.coarse is False
    with pytest.raises(RuntimeError, match="eqlb_hierarchy_set_coarse"):
        ml.coarse_rows
    assert np.array_equal(bits(ml.precondition(r)), bits(before))
    ml.close()


# ---- 6. switching, the snapshot, the default ---------------------------------------------------------------------------------
@pytest.mark.parametrize("problem,p", [("poisson", 2), ("elasticity", 1)])
def test_switching_on_and_off(problem, p):
    """off: the bits of a handle that never saw the switch; on again: the factor is formed again, the same bits"""
    from dolfinx_eqlb_amd import cpp
    c = case(problem, "graded8", p)
    r = np.random.default_rng(4).standard_normal(c["ops"][-1].fixed.size)
    never = cpp.Multilevel(c["hs"], c["refs"])
    untouched = never.precondition(r)
    never.close()
    assert np.array_equal(bits(untouched), bits(c["H0"].precondition(r)))
    want = c["HC"][False].precondition(r)
    ml = cpp.Multilevel(c["hs"], c["refs"])
    assert ml.coarse is False
    for turn in range(2):   # (the second switch-on finds the memory allocated)
        ml.coarse = True
        ml.set_coarse(True)   # factors again
        assert ml.coarse is True
        assert np.array_equal(bits(ml.precondition(r)), bits(want))
        ml.coarse = False
        ml.set_coarse(0)
        assert ml.coarse is False
        assert np.array_equal(bits(ml.precondition(r)), bits(untouched))
    ml.close()


def test_a_new_mask_on_level_0_needs_another_set_coarse():
    from dolfinx_eqlb_amd import cpp
    c = case("poisson", "three", 2)
    dms = device_levels("three")[0]
    mesh = dms[0].mesh
    bf = mesh.boundary_facets()
    part = bf[:bf.size // 2]
    h0 = gm.make_handle("poisson", dms[0], 2, c["coeff"][0], (bf,))
    ml = cpp.Multilevel([h0] + c["hs"][1:], c["refs"], coarse=True)
    same_factor(ml, c["HC"][False])
    op0 = mc.poisson_op(mesh, 2, c["coeff"][0], part)
    H = Hierarchy([op0] + c["ops"][1:], c["refs"], coarse=True)
    assert H.coarse_factor()[0].size > c["HC"][False].coarse_factor()[0].size   # (the arrays grow)
    h0.set_dirichlet(part)
    ml.set_coarse(True)
    same_factor(ml, H)
    r = np.random.default_rng(9).standard_normal(c["ops"][-1].fixed.size)
    assert np.array_equal(bits(ml.precondition(r)), bits(H.precondition(r)))
    ml.close()


# ---- 7. a caller's stream, the pybind carrier ----------------------------------------------------------------------------------
def test_coarse_calls_on_a_user_stream():
    """The factor is formed, and the input exists, only late on the caller's non-blocking stream (behind a spin kernel);
    the input is gone right behind the call: everything is ordered on THAT stream."""
    import torch
    from dolfinx_eqlb_amd import cpp
    c = case("poisson", "graded8", 2)
    H, op = c["HC"][False], c["ops"][-1]
    r = np.random.default_rng(21).standard_normal(op.ndofs)
    b = lc.rhs(op)
    ref_u, ref_info = c["ml"].solve(b, np.zeros(op.ndofs), rtol=1e-8, maxit=2000)
    n = H.coarse_factor()[0].size
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    r_src, b_src = torch.from_numpy(r).to(dev), torch.from_numpy(b).to(dev)
    r_dev, b_dev = torch.full_like(r_src, float("nan")), torch.full_like(b_src, float("nan"))
    z_dev, x_dev = torch.full_like(r_src, float("nan")), torch.full_like(r_src, float("nan"))
    rows_dev = torch.full((n,), 7, dtype=torch.int32, device=dev)
    d_dev = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    W_dev = torch.full((n, n), float("nan"), dtype=torch.float64, device=dev)
    ml = cpp.Multilevel(c["hs"], c["refs"])
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(40_000_000)
        ml.set_coarse(True, stream=s.cuda_stream)
        ml.coarse_factor_raw(rows_dev.data_ptr(), d_dev.data_ptr(), W_dev.data_ptr(), n, stream=s.cuda_stream)
        r_dev.copy_(r_src)
        ml.precondition_raw(r_dev.data_ptr(), z_dev.data_ptr(), stream=s.cuda_stream)
        z = z_dev.clone()
        r_dev.fill_(float("nan"))
        torch.cuda._sleep(40_000_000)
        b_dev.copy_(b_src)
        x_dev.zero_()
        info = ml.solve_raw(b_dev.data_ptr(), x_dev.data_ptr(), 1e-8, 0.0, 2000, stream=s.cuda_stream)
        x = x_dev.clone()
        b_dev.fill_(float("nan"))
    s.synchronize()
    rows, d, W = H.coarse_factor()
    assert np.array_equal(rows_dev.cpu().numpy(), rows)
    assert np.array_equal(bits(d_dev.cpu().numpy()), bits(d)) and np.array_equal(bits(W_dev.cpu().numpy()), bits(W))
    assert np.array_equal(bits(z.cpu().numpy()), bits(H.precondition(r)))
    assert info == ref_info and np.array_equal(bits(x.cpu().numpy()), bits(ref_u))
    ml.close()


def test_pybind_carrier_equals_the_ctypes_route():
    from dolfinx_eqlb_amd import _cpp as cm
    from dolfinx_eqlb_amd import cpp
    mesh = create_unit_square(4)
    dm = cpp.DeviceMesh.from_cells(mesh.x, mesh.cell_nodes)
    base = cm.Mesh.from_cells(mesh.x[:, :2], mesh.cell_nodes)
    dms, refs, ms, trs = [dm], [], [base], []
    for _ in range(3):
        marked = lc.graded_marks(dms[-1].mesh)
        refs.append(dms[-1].refine(marked, keep_plan=True))
        dms.append(refs[-1].dmesh)
        new, parent_cell, _, _, tr = ms[-1].refine(marked, keep_plan=True)
        assert np.array_equal(parent_cell, refs[-1].parent_cell)
        ms.append(new)
        trs.append(tr)
    hs, ss = [], []
    for d, m in zip(dms, ms):
        facets = d.boundary_facets()
        hs.append(cpp.PrimalPoisson(d, 2))
        hs[-1].set_dirichlet(facets)
        ss.append(cm.PrimalPoisson(m, 2))
        ss[-1].set_dirichlet(facets)
    ml = cpp.Multilevel(hs, refs, local=True, coarse=True)
    r = np.random.default_rng(2).standard_normal(hs[-1].ndofs)
    rows, d, W = ml.coarse_factor()
    plain = cm.Multilevel(ss, trs)
    assert plain.coarse is False
    with pytest.raises(RuntimeError, match="eqlb_hierarchy_set_coarse"):
        plain.coarse_factor()
    z_plain = plain.precondition(r)
    for carrier in (cm.Multilevel(ss, trs, local=True, coarse=True), plain):
        carrier.local = True
        carrier.coarse = True
        assert carrier.coarse is True and carrier.coarse_rows == ml.coarse_rows == rows.size
        crows, cd, cW = carrier.coarse_factor()
        assert crows.dtype == np.int32 and np.array_equal(crows, rows)
        assert np.array_equal(bits(cd), bits(d)) and cW.shape == W.shape and np.array_equal(bits(cW), bits(W))
        assert np.array_equal(bits(carrier.precondition(r)), bits(ml.precondition(r)))
    plain.coarse = False
    plain.local = False
    assert np.array_equal(bits(plain.precondition(r)), bits(z_plain))
    assert not np.array_equal(bits(z_plain), bits(ml.precondition(r)))
    ml.close()
