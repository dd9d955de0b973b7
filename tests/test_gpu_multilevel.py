"""The multilevel preconditioner on the device (cpp.Multilevel, csrc/eqlb_multilevel.hip, k_restrict of
csrc/eqlb_transfer.hip) against its numpy statement (dolfinx_eqlb_amd/lsolver/multilevel.py: Hierarchy,
mesh/transfer.py: restrict_lagrange): restriction and preconditioner bit for bit in both memory spaces; the solve against
a direct solve with the bounds of check_solution, against the statement's iteration count and against the Jacobi entry on
the same handle; limits, refusals, a caller's stream; the growth of the count with the level; the adaptive loop with a
hierarchy that grows by one level per step.

The hierarchy stands on the base mesh of tests/test_gpu_primal_solve.py, create_unit_square(9, shuffle_seed=3,
perturb=0.15) with 324 cells (more than one workgroup of 256): refined on the device at refine_cases.level_marks (403
cells, parents with 1, 2, 3 and 4 children) and then uniformly (1612 cells).  The coefficients of a level are those of
its parents.  The solves at p = 3, 4 use the first two levels (their direct solves stay small)."""

import numpy as np
import pytest

import elasticity_cases as ec
import galerkin as gk
import multilevel_cases as mc
import primal_cases as pc
from dolfinx_eqlb_amd.lsolver import primal
from dolfinx_eqlb_amd.lsolver.multilevel import Hierarchy
from dolfinx_eqlb_amd.mesh import create_unit_square
from test_gpu_primal_elasticity import MIXED
from test_gpu_primal_elasticity import check_solution as check_elasticity
from test_gpu_primal_solve import bits
from test_gpu_primal_solve import check_solution as check_poisson

pytestmark = pytest.mark.gpu

U = pc.U
_CACHE = {}


def allowance(iterations):
    """the existing allowance for the rounding of the inner products"""
    return max(2, iterations // 20)


def device_levels():
    """(DeviceMesh per level, Refinement per link) of the three levels, refined on the device with the plans kept"""
    if "levels" not in _CACHE:
        from dolfinx_eqlb_amd import cpp
        from refine_cases import level_marks
        base = create_unit_square(9, shuffle_seed=3, perturb=0.15)
        assert base.ncells == 324
        dms, refs = [cpp.DeviceMesh(base)], []
        for marks in (level_marks(base.ncells, 1), None):
            m = dms[-1].mesh
            refs.append(dms[-1].refine(mc.all_cells(m.ncells) if marks is None else marks, keep_plan=True))
            dms.append(refs[-1].dmesh)
        assert sorted(set(np.bincount(refs[0].parent_cell, minlength=324))) == [1, 2, 3, 4]
        assert [d.mesh.ncells for d in dms] == [324, 403, 1612]
        _CACHE["levels"] = (dms, refs)
    return _CACHE["levels"]


def hierarchy(problem, p, nlevels=3, bc="all"):
    """the statement, the handles, the Multilevel and the coefficients of one (problem, p, levels, boundary layout)"""
    key = (problem, p, nlevels, bc)
    if key not in _CACHE:
        from dolfinx_eqlb_amd import cpp
        dms, refs = device_levels()
        dms, refs = dms[:nlevels], refs[:nlevels - 1]
        meshes = [d.mesh for d in dms]
        links = [(r.parent_cell, r.node_parent_facet) for r in refs]
        ops, hs = [], []
        if problem == "poisson":
            coeff = mc.coefficients(meshes, links, pc.kappa_of)
            for dm, m, k in zip(dms, meshes, coeff):
                facets = m.boundary_facets() if bc == "all" else np.concatenate(gk.side_facets(m)[:2])
                ops.append(mc.poisson_op(m, p, k, facets))
                hs.append(cpp.PrimalPoisson(dm, p, k))
                hs[-1].set_dirichlet(facets)
        else:
            coeff = mc.coefficients(meshes, links, ec.pi1_of)
            for dm, m, k in zip(dms, meshes, coeff):
                types = [] if bc == "all" else MIXED
                ops.append(mc.elasticity_op(m, p, k, types))
                hs.append(cpp.PrimalElasticity(dm, p, cell_pi1=k))
                hs[-1].set_dirichlet(*ec.dirichlet_lists(gk.elasticity_facet_types(m, types)))
        _CACHE[key] = dict(H=Hierarchy(ops, refs), ml=cpp.Multilevel(hs, refs), hs=hs, ops=ops, coeff=coeff,
                           meshes=meshes)
    return _CACHE[key]


CASES = [("poisson", 1), ("poisson", 2), ("poisson", 3), ("poisson", 4), ("elasticity", 1), ("elasticity", 2),
         ("elasticity", 3), ("elasticity", 4)]


# ---- 1. bit for bit --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem,p", CASES)
def test_restrict_and_precondition_bit_for_bit_host_memory(problem, p):
    c = hierarchy(problem, p)
    H, ml = c["H"], c["ml"]
    rng = np.random.default_rng(3 * p)
    rs = [None] + [rng.standard_normal(H.ops[l].fixed.size) for l in (1, 2)]   # rs[l]: a vector of level l
    for call in range(2):   # a second call gives the same bits
        for level in (1, 0):
            r = rs[level + 1]
            assert np.array_equal(bits(ml.restrict(level, r)), bits(H.restrict(level, r)))
            assert np.array_equal(bits(ml.restrict(level, r, masked=False)), bits(H.restrict(level, r, masked=False)))
        z = ml.precondition(rs[2])
        assert np.array_equal(bits(z), bits(H.precondition(rs[2])))
        assert np.all(z[H.ops[-1].fixed] == 0.0)


@pytest.mark.parametrize("problem,p", CASES)
def test_restrict_and_precondition_bit_for_bit_device_memory(problem, p):
    import torch
    c = hierarchy(problem, p)
    H, ml = c["H"], c["ml"]
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(5 * p)
    r = rng.standard_normal(H.ops[2].fixed.size)
    d_r = torch.from_numpy(r).to(dev)
    d_c = torch.full((H.ops[1].fixed.size,), float("nan"), dtype=torch.float64, device=dev)
    d_z = torch.full_like(d_r, float("nan"))
    torch.cuda.synchronize()
    for call in range(2):
        ml.restrict_raw(1, d_r.data_ptr(), d_c.data_ptr(), True)
        assert np.array_equal(bits(d_c.cpu().numpy()), bits(H.restrict(1, r)))
        ml.precondition_raw(d_r.data_ptr(), d_z.data_ptr())
        assert np.array_equal(bits(d_z.cpu().numpy()), bits(H.precondition(r)))
        assert np.array_equal(bits(d_r.cpu().numpy()), bits(r))   # the input is not touched


def test_a_new_mask_takes_effect_at_the_next_call():
    c = hierarchy("poisson", 2)
    H, ml, hs, ops = c["H"], c["ml"], c["hs"], c["ops"]
    r = np.random.default_rng(8).standard_normal(ops[2].ndofs)
    all_around = [m.boundary_facets() for m in c["meshes"]]
    try:
        for op, h, m in zip(ops, hs, c["meshes"]):
            part = gk.side_facets(m)[0]
            op.set_dirichlet(part)
            h.set_dirichlet(part)
        assert np.array_equal(bits(ml.precondition(r)), bits(H.precondition(r)))
    finally:
        for op, h, f in zip(ops, hs, all_around):
            op.set_dirichlet(f)
            h.set_dirichlet(f)
    assert np.array_equal(bits(ml.precondition(r)), bits(H.precondition(r)))


# ---- 2. the solve --------------------------------------------------------------------------------------------------------
def solve_and_check(problem, p, nlevels, bc, seed):
    c = hierarchy(problem, p, nlevels, bc)
    H, ml, op, h = c["H"], c["ml"], c["ops"][-1], c["hs"][-1]
    n = op.fixed.size
    rng = np.random.default_rng(seed)
    b = rng.standard_normal(n)
    u0 = np.where(op.fixed, rng.standard_normal(n), 0.0) if bc == "mixed" else np.zeros(n)
    start = np.where(op.fixed, u0, rng.standard_normal(n)) if bc == "mixed" else u0
    u, info = ml.solve(b, start, rtol=1e-10, maxit=5000)
    if problem == "poisson":
        check_poisson(op, pc.assemble(c["meshes"][-1], p, c["coeff"][-1])[0], b, u0, u, info, 1e-10)
    else:
        check_elasticity(op, ec.assemble(c["meshes"][-1], p, 1.0, c["coeff"][-1])[0], b, u0, u, info, 1e-10)
    _, si = H.pcg(b, start, rtol=1e-10, maxit=5000)
    _, ji = h.solve(b, start, rtol=1e-10, maxit=20000)
    print(f"{problem} p={p} {nlevels} levels {bc}: hierarchy {info['iterations']} iterations, statement "
          f"{si['iterations']}, Jacobi entry {ji['iterations']}")
    assert abs(si["iterations"] - info["iterations"]) <= allowance(info["iterations"])
    assert ji["converged"] == 1 and info["iterations"] < ji["iterations"]
    u2, info2 = ml.solve(b, start, rtol=1e-10, maxit=5000)
    assert np.array_equal(bits(u), bits(u2)) and info == info2


@pytest.mark.parametrize("problem,p,nlevels", [("poisson", 1, 3), ("poisson", 2, 3), ("poisson", 3, 2), ("poisson", 4, 2),
                                               ("elasticity", 1, 3), ("elasticity", 2, 2)])
def test_solve_dirichlet_all_around(problem, p, nlevels):
    solve_and_check(problem, p, nlevels, "all", 11 * p)


@pytest.mark.parametrize("problem,p,nlevels", [("poisson", 1, 3), ("poisson", 2, 2), ("poisson", 3, 2), ("poisson", 4, 2),
                                               ("elasticity", 1, 3), ("elasticity", 2, 2)])
def test_solve_mixed_boundary(problem, p, nlevels):
    """Dirichlet values on two sides (Poisson) / the layout MIXED of the elasticity tests, any start on the free rows"""
    solve_and_check(problem, p, nlevels, "mixed", 13 * p)


@pytest.mark.parametrize("problem,p", [("poisson", 2), ("elasticity", 1)])
def test_one_level_is_jacobi(problem, p):
    from dolfinx_eqlb_amd import cpp
    c = hierarchy(problem, p)
    op, h = c["ops"][1], c["hs"][1]
    ml = cpp.Multilevel([h], [])
    n = op.fixed.size
    rng = np.random.default_rng(2)
    r, b = rng.standard_normal(n), rng.standard_normal(n)
    assert np.array_equal(bits(ml.precondition(r)), bits(np.where(op.fixed, 0.0, r / op.diagonal())))
    u, info = ml.solve(b, np.zeros(n), rtol=1e-10, maxit=20000)
    uj, ji = h.solve(b, np.zeros(n), rtol=1e-10, maxit=20000)
    print(f"{problem} p={p}: one level {info['iterations']} iterations, Jacobi entry {ji['iterations']}")
    assert info["converged"] == 1 and abs(info["iterations"] - ji["iterations"]) <= allowance(ji["iterations"])
    assert np.abs(u - uj).max() <= 1e-8 * np.abs(uj).max()
    with pytest.raises(RuntimeError, match="level = 0 outside"):
        ml.restrict(0, r)
    ml.close()


# ---- 3. limits, refusals, streams ----------------------------------------------------------------------------------------
def test_limits():
    c = hierarchy("poisson", 2)
    H, ml, op = c["H"], c["ml"], c["ops"][-1]
    b = np.random.default_rng(1).standard_normal(op.ndofs)
    u0 = np.zeros(op.ndofs)
    u3, i3 = ml.solve(b, u0, rtol=1e-10, maxit=3)
    s3, j3 = H.pcg(b, u0, rtol=1e-10, maxit=3)
    assert i3["converged"] == 0 and i3["iterations"] == 3 and i3["breakdown"] == 0 and j3["iterations"] == 3
    assert np.abs(u3 - s3).max() <= 3 * 8 * op.ndofs * U * np.abs(s3).max()
    # maxit beyond one batch of iterations between two reads of the state
    _, i11 = ml.solve(b, u0, rtol=1e-10, maxit=11)
    assert i11["converged"] == 0 and i11["iterations"] == 11
    # already solved: no iteration; nothing to solve: u^
    u1, i1 = ml.solve(b, u0, rtol=1e-10, maxit=5000)
    u4, i4 = ml.solve(b, u1, rtol=1e-9, maxit=50)
    assert i4["iterations"] == 0 and i4["converged"] == 1 and np.array_equal(bits(u4), bits(u1))
    u5, i5 = ml.solve(np.zeros(op.ndofs), np.where(op.fixed, 0.0, 1.0), rtol=0.0, atol=0.0, maxit=5)
    assert i5["converged"] == 1 and i5["iterations"] == 0 and np.all(u5 == 0.0)
    # a NaN in b: breakdown within maxit
    bn = b.copy()
    bn[np.nonzero(~op.fixed)[0][7]] = np.nan
    _, i6 = ml.solve(bn, u0, rtol=1e-10, maxit=40)
    assert i6["breakdown"] == 1 and i6["converged"] == 0 and i6["iterations"] <= 40
    for kw in (dict(maxit=0), dict(rtol=-1.0), dict(atol=float("nan"))):
        with pytest.raises(RuntimeError, match="eqlb_hierarchy_solve"):
            ml.solve(b, u0, **kw)
    # the next valid call works
    u7, i7 = ml.solve(b, u0, rtol=1e-10, maxit=5000)
    assert np.array_equal(bits(u7), bits(u1)) and i7 == i1


def test_refusals():
    from dolfinx_eqlb_amd import cpp
    dms, refs = device_levels()
    c = hierarchy("poisson", 2)
    hs, ml, op = c["hs"], c["ml"], c["ops"][-1]
    other_p = hierarchy("poisson", 1)["hs"]
    el = hierarchy("elasticity", 1)["hs"]
    with pytest.raises(RuntimeError, match="levels of different p"):
        cpp.Multilevel([hs[0], other_p[1], hs[2]], refs)
    with pytest.raises(RuntimeError, match="plan 0 "):
        cpp.Multilevel(hs, [refs[1], refs[0]])
    with pytest.raises(RuntimeError, match="plan 0 "):
        cpp.Multilevel([hs[0], hs[2]], [refs[0]])
    with pytest.raises(RuntimeError, match="not a mixture"):
        cpp.Multilevel([hs[0], el[1], hs[2]], refs)
    closed = dms[0].refine(np.array([0], dtype=np.int32))
    with pytest.raises(RuntimeError, match="plan of the refinement was not kept"):
        cpp.Multilevel([hs[0], hs[1]], [closed])
    # a solver whose mesh is not that of its level (the raw entry: the binding takes the mesh from the solver)
    import ctypes as C
    L = cpp.lib()
    out = C.c_void_p()
    sv = (C.c_void_p * 2)(hs[1]._h.value, hs[1]._h.value)
    ms = (C.c_void_p * 2)(dms[0]._h.value, dms[1]._h.value)
    pl = (C.c_void_p * 1)(refs[0].plan._h.value)
    assert L.eqlb_hierarchy_create(C.c_int32(2), C.c_int32(1), sv, pl, ms, None, C.byref(out)) == -1
    assert "the solver of level 0" in L.eqlb_last_error().decode() and not out.value
    r = np.ones(op.ndofs)
    for level in (-1, 2, 7):
        with pytest.raises(RuntimeError, match=f"level = {level} outside 0 ... 1"):
            ml.restrict(level, r)
    z = np.zeros(op.ndofs)
    for call in (lambda: ml.restrict_raw(0, r.ctypes.data, z.ctypes.data, True, 5),
                 lambda: ml.precondition_raw(r.ctypes.data, z.ctypes.data, 5),
                 lambda: ml.solve_raw(r.ctypes.data, z.ctypes.data, memspace=-1)):
        with pytest.raises(RuntimeError, match="unknown memory space"):
            call()
    with pytest.raises(RuntimeError, match="Input sizes does not match"):
        ml.precondition(r[:-1])
    singular = cpp.PrimalPoisson(dms[2], 2)
    with pytest.raises(RuntimeError, match="singular"):
        cpp.Multilevel([hs[0], hs[1], singular], refs).solve(r, z)
    # the next valid call works
    assert np.array_equal(bits(ml.precondition(r)), bits(c["H"].precondition(r)))


def test_precondition_and_solve_on_a_user_stream():
    """The inputs exist only late on the caller's non-blocking stream (behind a spin kernel; before that the buffers hold
    NaN) and are gone right behind the call: everything the calls enqueue is ordered on THAT stream."""
    import torch
    c = hierarchy("poisson", 2)
    H, ml, op = c["H"], c["ml"], c["ops"][-1]
    rng = np.random.default_rng(21)
    r, b = rng.standard_normal(op.ndofs), rng.standard_normal(op.ndofs)
    ref_z = H.precondition(r)
    ref_u, ref_info = ml.solve(b, np.zeros(op.ndofs), rtol=1e-10, maxit=5000)
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    r_src, b_src = torch.from_numpy(r).to(dev), torch.from_numpy(b).to(dev)
    r_dev, b_dev = torch.full_like(r_src, float("nan")), torch.full_like(b_src, float("nan"))
    z_dev, x_dev = torch.full_like(r_src, float("nan")), torch.full_like(r_src, float("nan"))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(40_000_000)
        r_dev.copy_(r_src)
        ml.precondition_raw(r_dev.data_ptr(), z_dev.data_ptr(), stream=s.cuda_stream)
        z = z_dev.clone()
        r_dev.fill_(float("nan"))
        torch.cuda._sleep(40_000_000)
        b_dev.copy_(b_src)
        x_dev.zero_()
        info = ml.solve_raw(b_dev.data_ptr(), x_dev.data_ptr(), 1e-10, 0.0, 5000, stream=s.cuda_stream)
        x = x_dev.clone()
        b_dev.fill_(float("nan"))
        x_dev.fill_(float("nan"))
    s.synchronize()
    assert np.array_equal(bits(z.cpu().numpy()), bits(ref_z))
    assert info == ref_info and np.array_equal(bits(x.cpu().numpy()), bits(ref_u))


# ---- 4. growth with the level -----------------------------------------------------------------------------------------------
def test_iterations_hardly_grow_with_the_level():
    """P_1 with kappa = 1 on uniformly refined levels of create_unit_square(2, ...), 16 * 4^L cells, rtol 1e-8 from
    zero: from L = 3 (1 024 cells) to L = 5 (16 384 cells) the count of the hierarchy grows by at most 1.5, that of the
    Jacobi entry by at least 2.  The statement gives 27 -> 34 and 80 -> 310 (tests/test_multilevel_host.py)."""
    from dolfinx_eqlb_amd import cpp
    dms, refs, hs = [cpp.DeviceMesh(create_unit_square(2, shuffle_seed=3, perturb=0.15))], [], []
    for level in range(6):
        m = dms[-1].mesh
        hs.append(cpp.PrimalPoisson(dms[-1], 1))
        hs[-1].set_dirichlet(m.boundary_facets())
        if level < 5:
            refs.append(dms[-1].refine(mc.all_cells(m.ncells), keep_plan=True))
            dms.append(refs[-1].dmesh)
    counts = {}
    for L in (3, 5):
        ml = cpp.Multilevel(hs[:L + 1], refs[:L])
        n = hs[L].ndofs
        b = np.random.default_rng(L).standard_normal(n)
        _, info = ml.solve(b, np.zeros(n), rtol=1e-8, maxit=5000)
        _, ji = hs[L].solve(b, np.zeros(n), rtol=1e-8, maxit=5000)
        assert info["converged"] == 1 and ji["converged"] == 1
        counts[L] = (info["iterations"], ji["iterations"])
        print(f"L = {L}: {dms[L].mesh.ncells} cells, hierarchy {counts[L][0]} iterations, Jacobi entry {counts[L][1]}")
        ml.close()
    assert counts[5][0] <= 1.5 * counts[3][0]
    assert counts[5][1] >= 2 * counts[3][1]


# ---- 5. the loop ------------------------------------------------------------------------------------------------------------
def test_adaptive_loop_with_a_growing_hierarchy():
    """The loop of tests/test_gpu_primal_solve.py at k = 2 - project_dg, load, solve from the prolonged u,
    primal_flux_dg, equilibrate, estimate, oscillation, indicator_total, mark_doerfler(0.5), refine(keep_plan),
    child_facets, prolong - with the solve through a Multilevel over all levels so far: one level more per step.  Every
    level's solve meets the bounds of check_solution against a direct solve."""
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
    from dolfinx_eqlb_amd.eqlb import check_eqlb_conditions as chk
    from synthetic import facet_types
    import test_estimator_bound as teb
    k = 2
    qp, qw = make_quadrature_triangle(2 * k + 6)
    dm = cpp.DeviceMesh(create_unit_square(4, shuffle_seed=3, perturb=0.15))
    facets = dm.mesh.boundary_facets()
    u = eq_old = None
    solvers, refs, keep, iters = [], [], [], []
    for level in range(3):
        mesh = dm.mesh
        J, detJ, K = chk.cell_geometry(mesh)
        x0 = mesh.x[mesh.cell_nodes[:, 0], :2]
        xq = x0[:, None, :] + np.einsum("cij,qj->cqi", J, qp)
        fq = teb.f_ex(xq[..., 0], xq[..., 1])
        fh = cpp.project_dg(dm, k - 1, qp, qw, fq[None, :, :, None])[0]
        assert np.array_equal(np.sort(facets), np.sort(mesh.boundary_facets()))
        pp = cpp.PrimalPoisson(dm, k)
        pp.set_dirichlet(facets)
        solvers.append(pp)
        ml = cpp.Multilevel(solvers, refs)
        assert ml.nlevels == level + 1
        b = pp.load(k - 1, fh)
        start = np.zeros(pp.ndofs) if u is None else u
        u, info = ml.solve(b, start, rtol=1e-12, maxit=5000)
        op = primal.PoissonOperator(mesh, k)
        op.set_dirichlet(facets)
        check_poisson(op, pc.assemble(mesh, k)[0], b, np.where(op.fixed, start, 0.0), u, info, 1e-12)
        iters.append(info["iterations"])
        cd, ndofs = dm.lagrange_dofmap(k)
        G = cpp.primal_flux_dg(dm, k, k - 1, cd, u)[0]
        eq = cpp.SemiExplicitEquilibrator(dm, k, 1)
        if level == 0:
            eq.set_boundary(facet_types(mesh, None))
        else:
            eq.carry_boundary(eq_old, refs[-1])
        x = eq.equilibrate_host(G[None], fh[None])
        div2, sig2, jump = cpp.estimate(dm, k, x, G[None], fh[None])
        eta_osc2 = cpp.oscillation(dm, k, x, G[None], qp, qw, fq[None])[0]
        cell_eta2, totals = cpp.indicator_total([sig2[0], eta_osc2], pair_last_two=True)
        eta = float(np.sqrt(totals[-1]))
        err = gk.energy_error(mesh, k, u, gk.dofmap(mesh, k)[0], teb.grad_ex)
        print(f"level {level}: {mesh.ncells} cells, {ml.nlevels} levels, {info['iterations']} iterations, eta {eta:.6e}, "
              f"err {err:.6e}, effectivity {eta / err:.4f}")
        assert np.sqrt(div2.sum()) < 1e-9 * np.sqrt(np.sum(fh ** 2)) and jump.max() < 1e-9
        assert eta / err >= 1.0 - 1e-10
        keep.append((dm, eq, ml))   # the plans and the hierarchy read the old handles: they outlive the level
        if level == 2:
            break
        marked, _ = cpp.mark_doerfler(cell_eta2, 0.5)
        refs.append(dm.refine(marked, keep_plan=True))
        u = refs[-1].prolong(k, u)
        facets = refs[-1].child_facets(facets, flat=True)
        eq_old, dm = eq, refs[-1].dmesh
    print(f"iterations per level {iters}")
