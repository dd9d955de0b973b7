"""Local smoothing of the multilevel preconditioner on the device (cpp.Multilevel(..., local=True),
eqlb_hierarchy_set_local / _active / _active_count, k_ml_active and k_ml_combine_local of csrc/eqlb_multilevel.hip) against
its numpy statement (lsolver.multilevel.Hierarchy(..., local=True)): the active rows exactly, the preconditioner bit for
bit in both memory spaces and for several columns, the solves against the statement's count and a direct solve, the
switch, the refusals, a caller's stream, and the pybind carrier against the ctypes route.

The hierarchies: the graded one of tests/multilevel_local_cases.py, refined on the device (9 levels, 64 -> 1 817 cells:
levels of fewer and of more rows than one block of 256, the Dirichlet corner inside the refined region), and
lshape_graded and disk70 of tests/primal_mesh_cases.py through the builders of tests/test_gpu_primal_meshes.py."""

import numpy as np
import pytest

import multilevel_cases as mc
import multilevel_local_cases as lc
import primal_mesh_cases as pm
import test_gpu_primal_meshes as gm
from dolfinx_eqlb_amd.lsolver.multilevel import Hierarchy
from dolfinx_eqlb_amd.mesh import create_unit_square
from test_gpu_multilevel import allowance
from test_gpu_primal_elasticity import check_solution as check_elasticity
from test_gpu_primal_many import compare
from test_gpu_primal_solve import bits
from test_gpu_primal_solve import check_solution as check_poisson

pytestmark = pytest.mark.gpu

PS_THREADS = 256
NREF = 8
_CACHE = {}


def graded_levels():
    """(DeviceMesh per level, Refinement per link) of the graded hierarchy, refined on the device with the plans kept"""
    if "graded" not in _CACHE:
        from dolfinx_eqlb_amd import cpp
        dms, refs = [cpp.DeviceMesh(create_unit_square(4))], []
        for _ in range(NREF):
            refs.append(dms[-1].refine(lc.graded_marks(dms[-1].mesh), keep_plan=True))
            dms.append(refs[-1].dmesh)
        assert [dms[0].mesh.ncells, dms[-1].mesh.ncells] == [64, 1817]
        _CACHE["graded"] = (dms, refs)
    return _CACHE["graded"]


def local_case(problem, name, p):
    """the local statement HL, the local Multilevel ml on handles of its own, the full statement H, and the rest of the
    case (ops, hs, meshes, coeff), Dirichlet all around"""
    key = (problem, name, p)
    if key not in _CACHE:
        from dolfinx_eqlb_amd import cpp
        if name == "graded":
            dms, refs = graded_levels()
            meshes = [d.mesh for d in dms]
            links = [(r.parent_cell, r.node_parent_facet) for r in refs]
            coeff = mc.coefficients(meshes, links, pm.pc.kappa_of if problem == "poisson" else pm.ec.pi1_of)
            ops, hs = [], []
            for dm, m, k in zip(dms, meshes, coeff):
                op, _, args = pm.statement(problem, m, p, "all", k)
                ops.append(op)
                hs.append(gm.make_handle(problem, dm, p, k, args))
            c = dict(H=Hierarchy(ops, refs), hs=hs, ops=ops, coeff=coeff, meshes=meshes)
        else:
            c = dict(gm.hierarchy(problem, name, p))
            refs = gm.device_levels(name)[1]
        c["refs"] = refs
        c["HL"] = Hierarchy(c["ops"], refs, local=True)
        c["ml"] = cpp.Multilevel(c["hs"], refs, local=True)
        assert c["ml"].local is True
        _CACHE[key] = c
    return _CACHE[key]


ALL = [(problem, p) for problem in ("poisson", "elasticity") for p in (1, 2, 3, 4)]


# ---- 1. the active rows ----------------------------------------------------------------------------------------------------
def check_active(ml, HL):
    total = 0
    for level in range(HL.nlevels):
        want = HL.active(level)
        got = ml.active(level)
        assert got.dtype == bool and np.array_equal(got, want), level
        assert ml.active_count(level) == int(want.sum()), level
        total += int(want.sum())
    return total


@pytest.mark.parametrize("problem,p", ALL)
def test_active_rows_on_the_graded_hierarchy(problem, p):
    """every level, among them levels of fewer rows than one block and levels whose row count crosses a multiple of
    the block (a partial last block behind full ones)"""
    c = local_case(problem, "graded", p)
    HL, ml = c["HL"], c["ml"]
    n = [op.fixed.size for op in HL.ops]
    assert any(v > PS_THREADS and v % PS_THREADS for v in n)
    if p == 1:
        assert any(v < PS_THREADS for v in n)
    active = check_active(ml, HL)
    print(f"{problem} p={p}: rows per level {n}, {sum(n)} over all levels, {active} active")
    assert all(0 < HL.active(l).sum() < n[l] for l in range(1, HL.nlevels))


@pytest.mark.parametrize("bs", [1, 2])
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_active_rows_of_one_marked_cell_and_of_a_uniform_link(p, bs):
    """one marked cell: the active rows are those of the children of the marked cell and of the few cells of its
    closure (5 of 324 cells here); then a uniform link: all ones"""
    from dolfinx_eqlb_amd import cpp
    if "one" not in _CACHE:
        dm = cpp.DeviceMesh(create_unit_square(9, shuffle_seed=3, perturb=0.15))
        refs = [dm.refine(np.array([5], dtype=np.int32), keep_plan=True)]
        refs.append(refs[0].dmesh.refine(mc.all_cells(refs[0].dmesh.mesh.ncells), keep_plan=True))
        _CACHE["one"] = (dm, refs)
    dm, refs = _CACHE["one"]
    cut = int((np.bincount(refs[0].parent_cell) > 1).sum())
    assert cut == 5
    problem = "poisson" if bs == 1 else "elasticity"
    ops, hs = [], []
    for d in (dm, refs[0].dmesh, refs[1].dmesh):
        op, k, args = pm.statement(problem, d.mesh, p, "all")
        ops.append(op)
        hs.append(gm.make_handle(problem, d, p, k, args))
    HL = Hierarchy(ops, refs, local=True)
    ml = cpp.Multilevel(hs, refs, local=True)
    check_active(ml, HL)
    nd = (p + 1) * (p + 2) // 2
    assert 0 < ml.active_count(1) <= bs * nd * int((np.bincount(refs[0].parent_cell)[refs[0].parent_cell] > 1).sum())
    assert ml.active_count(0) == ops[0].fixed.size and np.all(ml.active(0))
    assert ml.active_count(2) == ops[2].fixed.size and np.all(ml.active(2))
    ml.close()


# ---- 2. the preconditioner, bit for bit ------------------------------------------------------------------------------------
def _bit_cases():
    return [(problem, name, p) for name in ("graded", "lshape_graded", "disk70") for problem, p in ALL]


@pytest.mark.parametrize("problem,name,p", _bit_cases())
def test_local_precondition_bit_for_bit(problem, name, p):
    """host memory; a second call gives the same bits; Dirichlet rows lie inside the active regions"""
    c = local_case(problem, name, p)
    H, HL, ml = c["H"], c["HL"], c["ml"]
    L = HL.nlevels - 1
    assert any((HL.active(l) & HL.ops[l].fixed).any() for l in range(1, L + 1))
    r = np.random.default_rng(pm.seed_of("local", problem, name, p)).standard_normal(HL.ops[-1].fixed.size)
    want = HL.precondition(r)
    for call in range(2):
        z = ml.precondition(r)
        assert np.array_equal(bits(z), bits(want))
    assert np.all(z[HL.ops[-1].fixed] == 0.0)
    if name != "disk70":   # (its second link is uniform: one locally refined level)
        assert not np.array_equal(bits(want), bits(H.precondition(r)))   # smoothing an inactive row would show


@pytest.mark.parametrize("problem,p", [("poisson", 3), ("elasticity", 2)])
def test_local_precondition_bit_for_bit_device_memory(problem, p):
    import torch
    c = local_case(problem, "graded", p)
    HL, ml = c["HL"], c["ml"]
    dev = torch.device("cuda:0")
    n = HL.ops[-1].fixed.size
    for r in (np.random.default_rng(7 * p).standard_normal(n), np.where(HL.ops[-1].fixed, 0.0, -0.0)):
        d_r = torch.from_numpy(r).to(dev)
        d_z = torch.full_like(d_r, float("nan"))
        torch.cuda.synchronize()
        ml.precondition_raw(d_r.data_ptr(), d_z.data_ptr())
        assert np.array_equal(bits(d_z.cpu().numpy()), bits(HL.precondition(r)))
        assert np.array_equal(bits(d_r.cpu().numpy()), bits(r))   # the input is not touched
    # the mask in device memory
    for level in (0, 3):
        d_a = torch.full((HL.ops[level].fixed.size + 5,), 7, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ml.active_raw(level, d_a.data_ptr(), d_a.numel())
        a = d_a.cpu().numpy()
        assert np.array_equal(a[:-5].astype(bool), HL.active(level)) and np.all(a[:-5] <= 1) and np.all(a[-5:] == 7)


@pytest.mark.parametrize("nrhs", [1, 3, 5])
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_local_precondition_many(p, nrhs):
    """column c has the bits of the single call (5: a second group of four columns); a NaN right-hand side in one
    column leaves the others alone"""
    c = local_case("poisson", "graded", p)
    HL, ml = c["HL"], c["ml"]
    n = HL.ops[-1].ndofs
    V = np.random.default_rng(pm.seed_of("local-many", p, nrhs)).standard_normal((nrhs, n))
    single = np.stack([ml.precondition(v) for v in V])
    assert np.array_equal(bits(single[0]), bits(HL.precondition(V[0])))
    assert np.array_equal(bits(ml.precondition_many(V)), bits(single))
    bad = nrhs // 2
    Vn = V.copy()
    Vn[bad, np.nonzero(~HL.ops[-1].fixed)[0][7]] = np.nan
    Z = ml.precondition_many(Vn)
    assert np.isnan(Z[bad]).any()
    others = [k for k in range(nrhs) if k != bad]
    assert np.array_equal(bits(Z[others]), bits(single[others]))


def test_many_entries_stay_refused_on_elasticity_handles():
    c = local_case("elasticity", "graded", 1)
    ml = c["ml"]
    V = np.zeros((2, c["ops"][-1].fixed.size))
    with pytest.raises(RuntimeError, match="eqlb_hierarchy_precondition_many.*Poisson handles"):
        ml.precondition_many(V)
    with pytest.raises(RuntimeError, match="eqlb_hierarchy_solve_many.*Poisson handles"):
        ml.solve_many(V, V)


# ---- 3. the solves ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem,name,p", [("poisson", "graded", 1), ("elasticity", "graded", 1),
                                            ("poisson", "lshape_graded", 2)])
def test_local_solve(problem, name, p):
    """rtol 1e-8 from zero: the count within the allowance of the statement's, the bounds of check_solution against a
    direct solve, two solves with the same bits"""
    c = local_case(problem, name, p)
    HL, ml, op = c["HL"], c["ml"], c["ops"][-1]
    n = op.fixed.size
    assert int((~op.fixed).sum()) <= 3000
    b, u0 = lc.rhs(op), np.zeros(n)
    u, info = ml.solve(b, u0, rtol=1e-8, maxit=2000)
    check = check_poisson if problem == "poisson" else check_elasticity
    check(op, pm.assembled(problem, c["meshes"][-1], p, c["coeff"][-1]), b, u0, u, info, 1e-8)
    _, si = HL.pcg(b, u0, rtol=1e-8, maxit=2000)
    print(f"{problem} {name} p={p}: local hierarchy {info['iterations']} iterations, statement {si['iterations']}")
    assert si["converged"] == 1 and abs(si["iterations"] - info["iterations"]) <= allowance(info["iterations"])
    u2, info2 = ml.solve(b, u0, rtol=1e-8, maxit=2000)
    assert np.array_equal(bits(u), bits(u2)) and info == info2


def test_local_solve_many():
    """three columns on the graded hierarchy at p = 2: bits and info of the single solves, which converge"""
    c = local_case("poisson", "graded", 2)
    ml, op = c["ml"], c["ops"][-1]
    rng = np.random.default_rng(pm.seed_of("local-solve-many"))
    B = rng.standard_normal((3, op.ndofs))
    B[1] *= 1e-3
    U0 = np.where(op.fixed, rng.standard_normal((3, op.ndofs)), 0.0)
    infos = compare(ml.solve_many, ml.solve, B, U0, rtol=1e-8, maxit=2000)
    assert all(i["converged"] == 1 for i in infos)
    r = op.residual(B[2], ml.solve_many(B, U0, rtol=1e-8, maxit=2000)[0][2])
    assert np.sqrt(np.sum(r * r)) <= 1e-8 * infos[2]["nb"] * (1.0 + op.ndofs * pm.pc.U)


def test_local_needs_no_more_iterations_at_p1_on_the_device():
    """the counts of the two rules on the same handles, printed; P_1: local <= full (tests/test_multilevel_local_host.py
    asserts the same of the statement)"""
    from dolfinx_eqlb_amd import cpp
    for problem in ("poisson", "elasticity"):
        c = local_case(problem, "graded", 1)
        op = c["ops"][-1]
        b, u0 = lc.rhs(op), np.zeros(op.fixed.size)
        full = cpp.Multilevel(c["hs"], c["refs"])
        _, fi = full.solve(b, u0, rtol=1e-8, maxit=2000)
        full.close()
        _, li = c["ml"].solve(b, u0, rtol=1e-8, maxit=2000)
        print(f"{problem} p=1: full BPX {fi['iterations']} iterations, local {li['iterations']}")
        assert fi["converged"] == 1 and li["converged"] == 1 and li["iterations"] <= fi["iterations"]


# ---- 4. the switch, refusals, a caller's stream ---------------------------------------------------------------------------
@pytest.mark.parametrize("problem,p", [("poisson", 2), ("elasticity", 1)])
def test_switching_on_and_off(problem, p):
    from dolfinx_eqlb_amd import cpp
    c = local_case(problem, "graded", p)
    H, HL = c["H"], c["HL"]
    r = np.random.default_rng(4).standard_normal(H.ops[-1].fixed.size)
    ml = cpp.Multilevel(c["hs"], c["refs"])
    assert ml.local is False
    before = ml.precondition(r)
    assert np.array_equal(bits(before), bits(H.precondition(r)))
    for turn in range(2):   # (the second switch-on finds the masks allocated)
        ml.local = True
        ml.set_local(True)   # idempotent
        assert ml.local is True
        assert np.array_equal(bits(ml.precondition(r)), bits(HL.precondition(r)))
        assert np.array_equal(ml.active(HL.nlevels - 1), HL.active(HL.nlevels - 1))
        ml.local = False
        ml.set_local(0)
        assert ml.local is False
        assert np.array_equal(bits(ml.precondition(r)), bits(before))
    ml.close()


def test_refusals():
    from dolfinx_eqlb_amd import cpp
    c = local_case("poisson", "graded", 2)
    HL, on = c["HL"], c["ml"]
    ml = cpp.Multilevel(c["hs"], c["refs"])
    for call in (lambda: ml.active(1), lambda: ml.active_count(1)):
        with pytest.raises(RuntimeError, match="eqlb_hierarchy_active.*eqlb_hierarchy_set_local"):
            call()
    for value in (2, -1, 7):
        with pytest.raises(RuntimeError, match=f"eqlb_hierarchy_set_local: local = {value} is not 0 or 1"):
            ml.set_local(value)
        assert ml.local is False
    ml.close()
    with pytest.raises(RuntimeError, match="eqlb_hierarchy_set_local: local = 2"):
        on.set_local(2)
    assert on.local is True
    for level in (-1, HL.nlevels):
        with pytest.raises(RuntimeError, match=f"eqlb_hierarchy_active: level = {level} outside 0 ... {HL.nlevels - 1}"):
            on.active(level)
        with pytest.raises(RuntimeError, match=f"eqlb_hierarchy_active_count: level = {level} outside"):
            on.active_count(level)
    out = np.full(HL.ops[1].ndofs, 7, dtype=np.uint8)
    with pytest.raises(RuntimeError, match="eqlb_hierarchy_active: capacity"):
        on.active_raw(1, out.ctypes.data, out.size - 1, cpp.MEM_HOST)
    with pytest.raises(RuntimeError, match="unknown memory space"):
        on.active_raw(1, out.ctypes.data, out.size, 5)
    assert np.all(out == 7)
    # the next valid call works
    r = np.ones(HL.ops[-1].ndofs)
    assert np.array_equal(bits(on.precondition(r)), bits(HL.precondition(r)))


def test_local_calls_on_a_user_stream():
    """The masks are written, and the input exists, only late on the caller's non-blocking stream (behind a spin
    kernel); the input is gone right behind the call: everything is ordered on THAT stream."""
    import torch
    from dolfinx_eqlb_amd import cpp
    c = local_case("poisson", "graded", 2)
    HL, op = c["HL"], c["ops"][-1]
    r = np.random.default_rng(21).standard_normal(op.ndofs)
    b = lc.rhs(op)
    ref_u, ref_info = c["ml"].solve(b, np.zeros(op.ndofs), rtol=1e-8, maxit=2000)
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    r_src, b_src = torch.from_numpy(r).to(dev), torch.from_numpy(b).to(dev)
    r_dev, b_dev = torch.full_like(r_src, float("nan")), torch.full_like(b_src, float("nan"))
    z_dev, x_dev = torch.full_like(r_src, float("nan")), torch.full_like(r_src, float("nan"))
    a_dev = torch.full((op.ndofs,), 7, dtype=torch.uint8, device=dev)
    ml = cpp.Multilevel(c["hs"], c["refs"])
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(40_000_000)
        ml.set_local(True, stream=s.cuda_stream)
        ml.active_raw(HL.nlevels - 1, a_dev.data_ptr(), a_dev.numel(), stream=s.cuda_stream)
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
    assert np.array_equal(a_dev.cpu().numpy().astype(bool), HL.active(HL.nlevels - 1))
    assert np.array_equal(bits(z.cpu().numpy()), bits(HL.precondition(r)))
    assert info == ref_info and np.array_equal(bits(x.cpu().numpy()), bits(ref_u))
    ml.close()


# ---- 5. the pybind carrier -------------------------------------------------------------------------------------------------
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
    ml = cpp.Multilevel(hs, refs, local=True)
    r = np.random.default_rng(2).standard_normal(hs[-1].ndofs)
    full = cm.Multilevel(ss, trs)
    assert full.local is False
    with pytest.raises(RuntimeError, match="eqlb_hierarchy_set_local"):
        full.active(1)
    z_full = full.precondition(r)
    for carrier in (cm.Multilevel(ss, trs, local=True), full):
        carrier.local = True
        assert carrier.local is True
        for level in range(4):
            a = carrier.active(level)
            assert a.dtype == bool and np.array_equal(a, ml.active(level))
            assert carrier.active_count(level) == ml.active_count(level)
        assert np.array_equal(bits(carrier.precondition(r)), bits(ml.precondition(r)))
    full.local = False
    assert np.array_equal(bits(full.precondition(r)), bits(z_full))
    assert not np.array_equal(bits(z_full), bits(ml.precondition(r)))
    ml.close()
