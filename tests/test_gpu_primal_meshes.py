"""The P_p solves and the multilevel preconditioner on the device (cpp.PrimalPoisson, cpp.PrimalElasticity,
cpp.Multilevel) against their numpy statements on the meshes of tests/primal_mesh_cases.py: a vertex of 100 cells, holes,
two components, a pinched vertex, an unstructured mesh, tiny, huge, far-from-origin and stretched cells, cell counts that
are whole workgroups, one and two cells, more rows than one pass of the streaming kernels, and hierarchies of up to nine
levels with levels below one block of the restriction.  The assertions are those of tests/test_gpu_primal_solve.py,
tests/test_gpu_primal_elasticity.py, tests/test_gpu_multilevel.py and tests/test_gpu_primal_many.py (bits, check_solution
and compare are imported from there); new are the inputs.  tests/test_primal_meshes_host.py holds the statements to an
assembled matrix on the same inputs.

A solve is capped at twice the statement's own iteration count (primal_mesh_cases.SINGLE_SOLVES, HIERARCHY_SOLVES): a cap
against a silent crawl, not a tolerance.  No solve here runs the statement's PCG again - the counts are in the table."""

import numpy as np
import pytest

import primal_mesh_cases as pm
from test_gpu_primal_elasticity import check_solution as check_elasticity
from test_gpu_primal_many import compare
from test_gpu_primal_solve import bits
from test_gpu_primal_solve import check_solution as check_poisson

pytestmark = pytest.mark.gpu

U = pm.pc.U
RTOL = 1e-10
_CACHE = {}


def device_mesh(name):
    if ("dm", name) not in _CACHE:
        from dolfinx_eqlb_amd import cpp
        _CACHE["dm", name] = cpp.DeviceMesh(pm.mesh_of(name))
    return _CACHE["dm", name]


def make_handle(problem, dm, p, coeff, args):
    from dolfinx_eqlb_amd import cpp
    h = cpp.PrimalPoisson(dm, p, coeff) if problem == "poisson" else cpp.PrimalElasticity(dm, p, cell_pi1=coeff)
    h.set_dirichlet(*args)
    return h


def single(problem, name, p, layout="all"):
    """the statement, the handle and the vectors of one (problem, mesh, p, boundary layout), made once"""
    key = (problem, name, p, layout)
    if key not in _CACHE:
        mesh = pm.mesh_of(name)
        op, coeff, args = pm.statement(problem, mesh, p, layout)
        h = make_handle(problem, device_mesh(name), p, coeff, args)
        assert h.ndofs == op.ndofs
        n = op.fixed.size
        c = dict(op=op, h=h, n=n, mesh=mesh, coeff=coeff, **pm.vectors(problem, mesh, p, n, name))
        c["b"] = op.load(c["d"], c["f"], c["e"])
        _CACHE[key] = c
    return _CACHE[key]


# ---- a. bit for bit, single level ------------------------------------------------------------------------------------------
def check_bits_host(c):
    op, h, u, b, n = c["op"], c["h"], c["u"], c["b"], c["n"]
    y, ym, bl, dg = op.apply(u), op.apply(u, masked=True), op.load(c["d"], c["f"]), op.diagonal()
    rs, nbs = op.residual(b, u), op.reference_norm(b, u)
    for call in range(2):   # a second call gives the same bits
        assert np.array_equal(bits(h.apply(u)), bits(y))
        assert np.array_equal(bits(h.apply(u, masked=True)), bits(ym))
        assert np.array_equal(bits(h.load(c["d"], c["f"])), bits(bl))
        assert np.array_equal(bits(h.load(c["d"], c["f"], c["e"])), bits(b))
        assert np.array_equal(bits(h.diagonal()), bits(dg))
        r, rn, nb = h.residual(b, u, norms=True)
        assert np.array_equal(bits(r), bits(rs))
        # the norms are sums in another order: n roundings
        assert abs(rn - np.sqrt(np.sum(rs * rs))) <= n * U * rn
        assert abs(nb - nbs) <= n * U * nb
        assert np.array_equal(bits(h.residual(b, u)), bits(rs))


def check_bits_device(c):
    import torch
    op, h, b, n = c["op"], c["h"], c["b"], c["n"]
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    u, bb, f, e = t(c["u"]), t(b), t(c["f"]), t(c["e"])
    out = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    norms = torch.full((2,), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    y, ym, bl, dg = op.apply(c["u"]), op.apply(c["u"], masked=True), op.load(c["d"], c["f"]), op.diagonal()
    rs, nbs = op.residual(b, c["u"]), op.reference_norm(b, c["u"])
    for call in range(2):
        h.apply_raw(u.data_ptr(), out.data_ptr(), False)
        assert np.array_equal(bits(out.cpu().numpy()), bits(y))
        h.apply_raw(u.data_ptr(), out.data_ptr(), True)
        assert np.array_equal(bits(out.cpu().numpy()), bits(ym))
        h.load_raw(c["d"], f.data_ptr(), e.data_ptr(), out.data_ptr())
        assert np.array_equal(bits(out.cpu().numpy()), bits(b))
        h.load_raw(c["d"], f.data_ptr(), None, out.data_ptr())
        assert np.array_equal(bits(out.cpu().numpy()), bits(bl))
        h.diagonal_raw(out.data_ptr())
        assert np.array_equal(bits(out.cpu().numpy()), bits(dg))
        h.residual_raw(bb.data_ptr(), u.data_ptr(), out.data_ptr(), norms.data_ptr())
        assert np.array_equal(bits(out.cpu().numpy()), bits(rs))
        nv = norms.cpu().numpy()
        assert abs(nv[0] - np.sqrt(np.sum(rs * rs))) <= n * U * nv[0]
        assert abs(nv[1] - nbs) <= n * U * nv[1]
    assert np.array_equal(bits(u.cpu().numpy()), bits(c["u"]))   # the input is not touched


def _bit_cases():
    out = []
    for problem, names in (("poisson", pm.SINGLE),
                           ("elasticity", ["disk100", "bowtie", "tiny_far", "aspect1000", "wg128", "wg256"])):
        for name in names:
            for p in (1, 2, 3, 4):
                out.append((problem, name, p, "all", "host"))
                if name in ("disk100", "aspect1000"):
                    out.append((problem, name, p, "all", "device"))
    out += [("poisson", "hole", p, "inner", "host") for p in (1, 2, 3, 4)]
    return out


@pytest.mark.parametrize("problem,name,p,layout,space", _bit_cases())
def test_statements_bit_for_bit(problem, name, p, layout, space):
    c = single(problem, name, p, layout)
    if layout == "inner":
        fixed = c["op"].fixed
        assert fixed.any() and (~fixed).sum() > fixed.sum()
    (check_bits_host if space == "host" else check_bits_device)(c)


# ---- b. the smallest meshes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,p,free,iterations", pm.SMALLEST)
def test_one_and_two_cells(name, p, free, iterations):
    c = single("poisson", name, p)
    op, h = c["op"], c["h"]
    assert int((~op.fixed).sum()) == free
    check_bits_host(c)
    b, u0, start = pm.solve_data(op, "poisson", name, p, True)
    if not free:
        u, info = h.solve(b, start, rtol=RTOL, maxit=5)
        assert info["iterations"] == 0 and info["converged"] == 1 and info["breakdown"] == 0
        assert np.array_equal(bits(u), bits(start))
        return
    u, info = h.solve(b, start, rtol=RTOL, maxit=2 * iterations)
    check_poisson(op, pm.assembled("poisson", c["mesh"], p, c["coeff"]), b, u0, u, info, RTOL)
    print(f"{name} p={p}: {info['iterations']} iterations, statement {iterations}")
    assert abs(info["iterations"] - iterations) <= pm.allowance(iterations)


# ---- c. more rows than one pass of the streaming kernels -----------------------------------------------------------------------
@pytest.mark.parametrize("problem,p", [("poisson", 3), ("elasticity", 2)])
def test_more_than_one_pass_against_the_statement(problem, p):
    c = single(problem, "sq91", p)
    op, h, n = c["op"], c["h"], c["n"]
    assert n > pm.ROWS_PER_PASS
    check_bits_host(c)
    # maxit = 3: the third iterate of the statement up to the rounding of three steps (inner products of n terms)
    b, u0, _ = pm.solve_data(op, problem, "sq91", p)
    u3, i3 = h.solve(b, u0, rtol=RTOL, maxit=3)
    s3, j3 = op.pcg(b, u0, rtol=RTOL, maxit=3)
    assert i3["converged"] == 0 and i3["iterations"] == 3 and i3["breakdown"] == 0 and j3["iterations"] == 3
    dev = np.abs(u3 - s3).max() / np.abs(s3).max()
    print(f"{problem} p={p}: {n} rows, third iterate: deviation {dev:.2e}, bound {3 * 8 * n * U:.2e}")
    assert np.abs(u3 - s3).max() <= 3 * 8 * n * U * np.abs(s3).max()
    assert abs(i3["rnorm"] - j3["rnorm"]) <= 3 * 8 * n * U * j3["rnorm"]


# ---- d. solves, single level, Jacobi ---------------------------------------------------------------------------------------
def check_count(label, iterations, count, asserted):
    print(f"{label}: {iterations} iterations, statement {count}, allowance {pm.allowance(iterations)}"
          f"{'' if asserted else ' (printed only)'}")
    if asserted:
        assert abs(count - iterations) <= pm.allowance(iterations)


@pytest.mark.parametrize("case", pm.SINGLE_SOLVES, ids=pm.case_id)
def test_solve_single_level(case):
    problem, name, p, layout, count, asserted = case
    c = single(problem, name, p, layout)
    op, h = c["op"], c["h"]
    free = int((~op.fixed).sum())
    assert 0 < free <= 3000
    b, u0, start = pm.solve_data(op, problem, name, p, layout != "all")
    if layout != "all":
        assert np.abs(u0[op.fixed]).max() > 0.0    # inhomogeneous values on the Dirichlet part of the boundary
    u, info = h.solve(b, start, rtol=RTOL, maxit=2 * count)
    check = check_poisson if problem == "poisson" else check_elasticity
    check(op, pm.assembled(problem, c["mesh"], p, c["coeff"]), b, u0, u, info, RTOL)
    check_count(pm.case_id(case), info["iterations"], count, asserted)


# ---- e. hierarchies ----------------------------------------------------------------------------------------------------------
def device_levels(name):
    """(DeviceMesh per level, Refinement per link) of levels_of(name), refined on the device with the plans kept"""
    if ("levels", name) not in _CACHE:
        from dolfinx_eqlb_amd import cpp
        base, marks = pm.levels_of(name)
        dms, refs = [cpp.DeviceMesh(base)], []
        for mk in marks:
            refs.append(dms[-1].refine(mk(dms[-1].mesh), keep_plan=True))
            dms.append(refs[-1].dmesh)
        pm.check_levels(name, [d.mesh for d in dms], [(r.parent_cell, r.node_parent_facet) for r in refs])
        _CACHE["levels", name] = (dms, refs)
    return _CACHE["levels", name]


def hierarchy(problem, name, p, nlevels=None):
    """the statement, the handles and the Multilevel of the first nlevels levels (all), Dirichlet all around"""
    dms, refs = device_levels(name)
    nlevels = len(dms) if nlevels is None else nlevels
    key = ("hierarchy", problem, name, p, nlevels)
    if key not in _CACHE:
        from dolfinx_eqlb_amd import cpp
        from dolfinx_eqlb_amd.lsolver.multilevel import Hierarchy
        dms, refs = dms[:nlevels], refs[:nlevels - 1]
        meshes = [d.mesh for d in dms]
        links = [(r.parent_cell, r.node_parent_facet) for r in refs]
        first = pm.pc.kappa_of if problem == "poisson" else pm.ec.pi1_of
        coeff = pm.mc.coefficients(meshes, links, first)
        ops, hs = [], []
        for dm, m, k in zip(dms, meshes, coeff):
            op, _, args = pm.statement(problem, m, p, "all", k)
            ops.append(op)
            hs.append(make_handle(problem, dm, p, k, args))
        _CACHE[key] = dict(H=Hierarchy(ops, refs), ml=cpp.Multilevel(hs, refs), hs=hs, ops=ops, coeff=coeff,
                           meshes=meshes)
    return _CACHE[key]


def _hierarchy_bit_cases():
    out = []
    for name in ("disk70", "hole"):
        out += [("poisson", name, p) for p in (1, 2, 3, 4)] + [("elasticity", name, p) for p in (1, 2)]
    out += [("poisson", "lshape_graded", p) for p in (1, 2, 3, 4)] + [("elasticity", "lshape_graded", p) for p in (2, 3)]
    return out


@pytest.mark.parametrize("problem,name,p", _hierarchy_bit_cases())
def test_restrict_and_precondition_bit_for_bit(problem, name, p):
    """every link, masked and raw, and the preconditioner; lshape_graded at p = 4 in device memory, the rest in host
    memory"""
    c = hierarchy(problem, name, p)
    H, ml = c["H"], c["ml"]
    L = H.nlevels - 1
    rng = np.random.default_rng(pm.seed_of("restrict", problem, name, p))
    rs = [None] + [rng.standard_normal(H.ops[l].fixed.size) for l in range(1, L + 1)]   # rs[l]: a vector of level l
    if (name, p) == ("lshape_graded", 4):
        import torch
        dev = torch.device("cuda:0")
        d_top = torch.from_numpy(rs[L]).to(dev)
        d_z = torch.full_like(d_top, float("nan"))
        for call in range(2):
            for level in range(L - 1, -1, -1):
                d_r = torch.from_numpy(rs[level + 1]).to(dev)
                d_c = torch.full((H.ops[level].fixed.size,), float("nan"), dtype=torch.float64, device=dev)
                torch.cuda.synchronize()
                for masked in (True, False):
                    ml.restrict_raw(level, d_r.data_ptr(), d_c.data_ptr(), masked)
                    assert np.array_equal(bits(d_c.cpu().numpy()), bits(H.restrict(level, rs[level + 1], masked=masked)))
                assert np.array_equal(bits(d_r.cpu().numpy()), bits(rs[level + 1]))   # the input is not touched
            ml.precondition_raw(d_top.data_ptr(), d_z.data_ptr())
            assert np.array_equal(bits(d_z.cpu().numpy()), bits(H.precondition(rs[L])))
        return
    for call in range(2):   # a second call gives the same bits
        for level in range(L - 1, -1, -1):
            r = rs[level + 1]
            assert np.array_equal(bits(ml.restrict(level, r)), bits(H.restrict(level, r))), level
            assert np.array_equal(bits(ml.restrict(level, r, masked=False)), bits(H.restrict(level, r, masked=False))), level
        z = ml.precondition(rs[L])
        assert np.array_equal(bits(z), bits(H.precondition(rs[L])))
        assert np.all(z[H.ops[-1].fixed] == 0.0)


@pytest.mark.parametrize("case", pm.HIERARCHY_SOLVES, ids=pm.case_id)
def test_solve_with_the_hierarchy(case):
    problem, name, p, nlevels, count, asserted = case
    c = hierarchy(problem, name, p, nlevels)
    ml, op = c["ml"], c["ops"][-1]
    assert c["H"].nlevels == nlevels and 0 < int((~op.fixed).sum()) <= 3000
    b, u0, start = pm.solve_data(op, problem, name, p)
    u, info = ml.solve(b, start, rtol=RTOL, maxit=2 * count)
    check = check_poisson if problem == "poisson" else check_elasticity
    check(op, pm.assembled(problem, c["meshes"][-1], p, c["coeff"][-1]), b, u0, u, info, RTOL)
    check_count(pm.case_id(case), info["iterations"], count, asserted)
    u2, info2 = ml.solve(b, start, rtol=RTOL, maxit=2 * count)
    assert np.array_equal(bits(u), bits(u2)) and info == info2


def test_many_columns_on_nine_levels():
    """precondition_many and solve_many with three columns on lshape_graded at p = 2 are the single calls: bits and info"""
    case = [c for c in pm.HIERARCHY_SOLVES if c[:3] == ("poisson", "lshape_graded", 2)][0]
    c = hierarchy("poisson", "lshape_graded", 2)
    ml, op = c["ml"], c["ops"][-1]
    rng = np.random.default_rng(pm.seed_of("many", "lshape_graded", 2))
    V = rng.standard_normal((3, op.ndofs))
    assert np.array_equal(bits(ml.precondition_many(V)), bits(np.stack([ml.precondition(v) for v in V])))
    B = rng.standard_normal((3, op.ndofs))
    B[1] *= 1e-3
    U0 = np.where(op.fixed, rng.standard_normal((3, op.ndofs)), 0.0)
    infos = compare(ml.solve_many, ml.solve, B, U0, rtol=RTOL, maxit=2 * case[4])
    assert all(i["converged"] == 1 for i in infos)
