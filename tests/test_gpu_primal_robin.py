"""The Robin term of the P_p Poisson handle on the device (cpp.PrimalPoisson.set_robin; csrc/eqlb_primal_gather.inc,
eqlb_primal_solve.hip, eqlb_primal_matrix.hip): the rule is the bits of the numpy statement (dolfinx_eqlb_amd/lsolver/
primal.py: PoissonOperator.set_robin) everywhere - apply (masked and not), diagonal, residual, robin_weights (the
comparison with np.sqrt is the test that the device square root is correctly rounded), matrix and matrix_values at
p = 1 ... 4, the many-column forms, lists in device memory on a non-blocking stream, a three-level hierarchy with
carry_robin between the levels (restrict carries no Robin term, precondition does), and the flux condition
alpha (u_h - u_ext) handed to the equilibrator, against the oracle within the 1e-11 of tests/test_inhomogeneous_bc.py;
robin_flux at p = 1 ... 4 and nq = 1, 4, 64 in host and device memory, the NaN rows of ids a device-memory list skipped,
and what robin_list() and carry_robin do with a list that was given through set_robin_raw.

The cases: the 576-cell square of tests/test_gpu_primal_many.py with facet-wise random alpha in [0, 10] including exact
zeros - Robin on two sides, Dirichlet on one, Neumann on one, and the same without the Dirichlet side - and from
tests/primal_mesh_cases.py `triangle` (all three facets: every vertex lies in two Robin facets), `right1`, `bowtie`
(the pinched vertex lies in four), `hole` (the inner loop only), `wg256`, `tiny_far`, `huge`, and `sq91` at p = 3 (more
rows than one pass of the sum kernel).  No tolerance appears below except in the comparison with the oracle."""

import numpy as np
import pytest

import primal_cases as pc
import primal_mesh_cases as pm
import robin_cases as rb
from dolfinx_eqlb_amd.lsolver import primal
from test_gpu_primal_solve import bits

pytestmark = pytest.mark.gpu

_CACHE = {}
NAMES = ("square576", "square576_free", "triangle", "right1", "bowtie", "hole", "wg256", "tiny_far", "huge")


def layout(name):
    """(mesh, Robin facets in a shuffled order, alpha per facet, Dirichlet facets)"""
    if name.startswith("square576"):
        from dolfinx_eqlb_amd.mesh import create_unit_square
        mesh = create_unit_square(12, shuffle_seed=3, perturb=0.15)
        assert mesh.ncells == 576
        left, bottom, right, top = rb.sides(mesh)
        robin = np.concatenate([right, top])
        dirichlet = left if name == "square576" else np.zeros(0, dtype=np.int32)       # bottom: Neumann
    else:
        mesh = pm.mesh_of(name)
        robin = (pm.dirichlet_facets(mesh, "inner") if name == "hole" else mesh.boundary_facets()).astype(np.int32)
        dirichlet = np.zeros(0, dtype=np.int32)
    robin = robin[np.random.default_rng(5).permutation(robin.size)].astype(np.int32)
    return mesh, robin, rb.alpha_of(robin.size), dirichlet.astype(np.int32)


def case(name, p):
    """the statement and the handle of one (mesh, p), both with the Robin list and the mask"""
    if (name, p) not in _CACHE:
        from dolfinx_eqlb_amd import cpp
        if ("dm", name) not in _CACHE:
            _CACHE["dm", name] = (cpp.DeviceMesh(layout(name)[0]),) + layout(name)[1:]
        dm, robin, alpha, dirichlet = _CACHE["dm", name]
        mesh = dm.mesh
        kappa = pc.kappa_of(mesh.ncells)
        op = primal.PoissonOperator(mesh, p, kappa)
        h = cpp.PrimalPoisson(dm, p, kappa)
        for o in (op, h):
            o.set_dirichlet(dirichlet)
            o.set_robin(robin, facet_alpha=alpha)
        _CACHE[name, p] = dict(dm=dm, mesh=mesh, op=op, h=h, robin=robin, alpha=alpha, dirichlet=dirichlet, kappa=kappa)
    return _CACHE[name, p]


def check_pieces(c, matrix=True):
    op, h, mesh = c["op"], c["h"], c["mesh"]
    rng = np.random.default_rng(pm.seed_of("robin", mesh.ncells, op.p))
    u, b = rng.standard_normal(op.ndofs), rng.standard_normal(op.ndofs)
    assert np.array_equal(bits(h.robin_weights()), bits(op.robin_weights()))
    fn = mesh.facet_nodes[c["robin"]]
    dx, dy = mesh.x[fn[:, 1], 0] - mesh.x[fn[:, 0], 0], mesh.x[fn[:, 1], 1] - mesh.x[fn[:, 0], 1]
    assert np.array_equal(bits(h.robin_weights()), bits(c["alpha"] * np.sqrt(dx * dx + dy * dy)))
    assert np.array_equal(bits(h.apply(u)), bits(op.apply(u)))
    assert np.array_equal(bits(h.apply(u, masked=True)), bits(op.apply(u, masked=True)))
    assert np.array_equal(bits(h.diagonal()), bits(op.diagonal()))
    r, rn, nb = h.residual(b, u, norms=True)
    assert np.array_equal(bits(r), bits(op.residual(b, u)))
    assert abs(nb - op.reference_norm(b, u)) <= 1e-13 * nb     # (the lifting carries the facet term of the fixed rows)
    if matrix:
        ip, ix, v = h.matrix()
        rp, rx, rv = op.matrix()
        assert np.array_equal(ip, rp) and np.array_equal(ix, rx) and np.array_equal(bits(v), bits(rv))
        assert np.array_equal(bits(h.matrix_values(eliminate=True)), bits(op.matrix(eliminate=True)[2]))
        assert np.array_equal(bits(h.matrix_values()), bits(rv))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_operator_pieces_bit_for_bit(name, p):
    c = case(name, p)
    fresh = primal.PoissonOperator(c["mesh"], p, c["kappa"])
    u = np.random.default_rng(p).standard_normal(fresh.ndofs)
    assert not np.array_equal(c["op"].apply(u), fresh.apply(u))       # (the term is there)
    check_pieces(c)


def test_more_rows_than_one_pass():
    from dolfinx_eqlb_amd import cpp
    mesh = pm.mesh_of("sq91")
    robin = mesh.boundary_facets().astype(np.int32)
    alpha = rb.alpha_of(robin.size)
    op = primal.PoissonOperator(mesh, 3)
    assert op.ndofs > pm.ROWS_PER_PASS
    h = cpp.PrimalPoisson(cpp.DeviceMesh(mesh), 3)
    for o in (op, h):
        o.set_robin(robin, facet_alpha=alpha)
    check_pieces(dict(op=op, h=h, mesh=mesh, robin=robin, alpha=alpha), matrix=False)


@pytest.mark.parametrize("name", ["square576", "bowtie"])
@pytest.mark.parametrize("p", [1, 3])
def test_empty_list_is_a_fresh_handle_and_a_new_list_replaces_the_old(name, p):
    from dolfinx_eqlb_amd import cpp
    c = case(name, p)
    mesh, robin, alpha = c["mesh"], c["robin"], c["alpha"]
    op, fresh = primal.PoissonOperator(mesh, p, c["kappa"]), primal.PoissonOperator(mesh, p, c["kappa"])
    h = cpp.PrimalPoisson(c["dm"], p, c["kappa"])
    u = np.random.default_rng(2).standard_normal(op.ndofs)
    for o in (op, h):
        o.set_robin(robin[:5], alpha=3.0)
    assert np.array_equal(bits(h.apply(u)), bits(op.apply(u))) and h.robin_count() == 5
    for o in (op, h):
        o.set_robin(robin[3:], facet_alpha=alpha[3:])
    assert np.array_equal(bits(h.apply(u)), bits(op.apply(u))) and np.array_equal(bits(h.diagonal()), bits(op.diagonal()))
    h.set_robin([])
    assert np.array_equal(bits(h.apply(u)), bits(fresh.apply(u)))
    assert np.array_equal(bits(h.diagonal()), bits(fresh.diagonal())) and h.robin_count() == 0
    # all alpha = 0: the term is on, changes no value, and makes nothing definite
    h.set_robin(robin, alpha=0.0)
    assert np.array_equal(h.apply(u), fresh.apply(u)) and not np.any(h.robin_weights())
    with pytest.raises(RuntimeError, match="singular: no Dirichlet DOF"):
        h.solve(u, np.zeros_like(u))
    h.set_robin([])
    with pytest.raises(RuntimeError, match="singular: no Dirichlet DOF"):
        h.solve(u, np.zeros_like(u))


def test_refusals_in_host_memory_leave_the_handle_as_it_was():
    c = case("square576", 2)
    h, op, mesh, robin, alpha = c["h"], c["op"], c["mesh"], c["robin"], c["alpha"]
    u = np.random.default_rng(1).standard_normal(op.ndofs)
    interior = int(np.nonzero(np.diff(mesh.facet_cells_offsets) == 2)[0][0])
    for bad in (interior, -1, mesh.nfacets):
        lst = robin.copy()
        lst[4] = bad
        with pytest.raises(RuntimeError, match=r"facets\[4\] = %d is no boundary facet" % bad):
            h.set_robin(lst, facet_alpha=alpha)
    lst = robin.copy()
    lst[7] = lst[2]
    with pytest.raises(RuntimeError, match=r"facets\[7\] = %d is listed twice" % lst[2]):
        h.set_robin(lst, facet_alpha=alpha)
    for value in (-1.0, np.nan, np.inf):
        a = alpha.copy()
        a[3] = value
        with pytest.raises(RuntimeError, match=r"facet_alpha\[3\]"):
            h.set_robin(robin, facet_alpha=a)
        with pytest.raises(RuntimeError, match="alpha = .* is negative, NaN or infinite"):
            h.set_robin(robin, alpha=value)
    assert np.array_equal(bits(h.apply(u)), bits(op.apply(u))) and np.array_equal(bits(h.diagonal()), bits(op.diagonal()))
    assert np.array_equal(bits(h.robin_weights()), bits(op.robin_weights()))


# ---- many columns ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,p", [("square576", 1), ("square576", 4), ("bowtie", 2), ("triangle", 3)])
def test_apply_many_is_the_single_calls(name, p):
    c = case(name, p)
    h, op = c["h"], c["op"]
    for R in range(1, 6):
        Uc = np.random.default_rng(R).standard_normal((R, op.ndofs))
        for masked in (False, True):
            Y = h.apply_many(Uc, masked=masked)
            for k in range(R):
                assert np.array_equal(bits(Y[k]), bits(h.apply(Uc[k], masked=masked)))
                assert np.array_equal(bits(Y[k]), bits(op.apply(Uc[k], masked=masked)))


def same_info(a, b):
    return a.keys() == b.keys() and all(np.array_equal(bits(a[k]), bits(b[k])) for k in a)


@pytest.mark.parametrize("name,p", [("square576", 2), ("square576_free", 1), ("square576_free", 3), ("bowtie", 2)])
def test_solve_and_solve_many(name, p):
    """the Jacobi solve with the term: converged against the statement's operator, without a Dirichlet DOF too; column c
    of solve_many has the bits and the info of solve"""
    c = case(name, p)
    h, op = c["h"], c["op"]
    n = op.ndofs
    rng = np.random.default_rng(p)
    B = rng.standard_normal((5, n))
    U0 = np.where(op.fixed, rng.standard_normal((5, n)), 0.0)
    X, infos = h.solve_many(B, U0, rtol=1e-10, maxit=20000)
    for k in range(5):
        x, info = h.solve(B[k], U0[k], rtol=1e-10, maxit=20000)
        assert info["converged"] == 1 and info["breakdown"] == 0
        assert np.array_equal(bits(X[k]), bits(x)) and same_info(infos[k], info)
        r = op.residual(B[k], x)
        assert np.sqrt(np.sum(r * r)) <= 1.01e-10 * op.reference_norm(B[k], U0[k])
    _, iref = op.pcg(B[0], U0[0], rtol=1e-10, maxit=20000)
    assert abs(infos[0]["iterations"] - iref["iterations"]) <= max(2, iref["iterations"] // 20)


# ---- lists in device memory, a non-blocking stream -------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 3])
def test_device_memory_list_on_a_non_blocking_stream(p):
    import torch
    from dolfinx_eqlb_amd import cpp
    c = case("square576", p)
    op, mesh, robin, alpha = c["op"], c["mesh"], c["robin"], c["alpha"]
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)      # non-blocking: not ordered against the default stream
    h = cpp.PrimalPoisson(c["dm"], p, c["kappa"])
    h.set_dirichlet(c["dirichlet"])
    torch.cuda.synchronize()
    interior = int(np.nonzero(np.diff(mesh.facet_cells_offsets) == 2)[0][0])
    # ids that are no boundary facet are skipped in device memory: nothing is read out of range, the rest is taken
    lst = np.concatenate([robin, [-7, mesh.nfacets + 3, interior]]).astype(np.int32)
    al = np.concatenate([alpha, [1.0, 2.0, 3.0]])
    u = np.random.default_rng(p).standard_normal(op.ndofs)
    with torch.cuda.stream(st):
        d_f, d_a = torch.from_numpy(lst).to(dev), torch.from_numpy(al).to(dev)
        d_u = torch.from_numpy(u).to(dev)
        d_y = torch.full_like(d_u, float("nan"))
        d_w = torch.full((lst.size,), float("nan"), dtype=torch.float64, device=dev)
        h.set_robin_raw(lst.size, d_f.data_ptr(), 1.0, d_a.data_ptr(), cpp.MEM_DEVICE, st.cuda_stream)
        h.apply_raw(d_u.data_ptr(), d_y.data_ptr(), False, cpp.MEM_DEVICE, st.cuda_stream)
        assert h.robin_weights_raw(d_w.data_ptr(), lst.size, cpp.MEM_DEVICE, st.cuda_stream) == lst.size
    st.synchronize()
    assert np.array_equal(bits(d_y.cpu().numpy()), bits(op.apply(u)))
    w = d_w.cpu().numpy()
    assert np.array_equal(bits(w[:robin.size]), bits(op.robin_weights())) and not np.any(w[robin.size:])
    s = np.array([0.0, 0.3, 1.0])
    flux = h.robin_flux(u, s)
    assert np.array_equal(bits(flux[:robin.size]), bits(primal.robin_flux(mesh, p, robin, alpha, u, s)))
    assert np.all(np.isnan(flux[robin.size:]))


# ---- the hierarchy ---------------------------------------------------------------------------------------------------
def robin_hierarchy(p, free):
    """three levels built as in tests/test_gpu_multilevel.py, the Robin list carried by carry_robin; free: no Dirichlet
    side on any level (an all-Robin level 0)"""
    key = ("hier", p, free)
    if key not in _CACHE:
        import multilevel_cases as mc
        from dolfinx_eqlb_amd import cpp
        from dolfinx_eqlb_amd.lsolver import Hierarchy
        from dolfinx_eqlb_amd.mesh import refine
        from test_gpu_multilevel import device_levels
        dms, refs = device_levels()
        meshes = [d.mesh for d in dms]
        links = [(r.parent_cell, r.node_parent_facet) for r in refs]
        coeff = mc.coefficients(meshes, links, pc.kappa_of)
        ops, hs = [], []
        f, a = None, None
        for l, (dm, m, k) in enumerate(zip(dms, meshes, coeff)):
            left, bottom, right, top = rb.sides(m)
            op, h = primal.PoissonOperator(m, p, k), cpp.PrimalPoisson(dm, p, k)
            dirichlet = np.zeros(0, dtype=np.int32) if free else left
            op.set_dirichlet(dirichlet)
            h.set_dirichlet(dirichlet)
            if l == 0:
                f = np.concatenate([right, top]) if not free else m.boundary_facets().astype(np.int32)
                a = rb.alpha_of(f.size)
                h.set_robin(f, facet_alpha=a)
            else:
                f2, a2 = refs[l - 1].carry_robin(hs[-1], h)
                rf, ra = refine.carry_robin_list(meshes[l - 1], refs[l - 1].node_parent_facet, m, f, a)
                assert np.array_equal(f2, rf) and np.array_equal(bits(a2), bits(ra)) and f2.size >= f.size
                f, a = f2, a2
            op.set_robin(f, facet_alpha=a)
            assert np.array_equal(bits(h.robin_weights()), bits(op.robin_weights()))
            ops.append(op)
            hs.append(h)
        assert f.size > hs[0].robin_count()        # (the uniform refinement bisects every listed facet)
        _CACHE[key] = dict(H=Hierarchy(ops, refs), ml=cpp.Multilevel(hs, refs), hs=hs, ops=ops, refs=refs)
    return _CACHE[key]


@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("free", [False, True])
def test_hierarchy_restrict_and_precondition_bit_for_bit(p, free):
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.lsolver import Hierarchy
    c = robin_hierarchy(p, free)
    H, ml, ops = c["H"], c["ml"], c["ops"]
    rng = np.random.default_rng(7 * p)
    rs = [None] + [rng.standard_normal(ops[l].fixed.size) for l in (1, 2)]
    for level in (1, 0):
        r = rs[level + 1]
        got = ml.restrict(level, r)
        assert np.array_equal(bits(got), bits(H.restrict(level, r)))
        # the restriction carries no Robin term: the bits of a hierarchy whose levels never had one
        plain = [primal.PoissonOperator(o.mesh, p, o.w / o.adet) for o in ops]
        for q, o in zip(plain, ops):
            q.fixed = o.fixed
        assert np.array_equal(bits(got), bits(Hierarchy(plain, c["refs"]).restrict(level, r)))
    z = ml.precondition(rs[2])
    assert np.array_equal(bits(z), bits(H.precondition(rs[2])))
    # (the numpy statement of the dense factor takes seconds on the 1513 rows of level 0 at p = 3: coarse at p <= 2)
    for local, coarse in ((True, False), (False, True), (True, True))[:3 if p <= 2 else 1]:
        ml.set_local(local)
        ml.set_coarse(coarse)
        Hv = Hierarchy(ops, c["refs"], local=local, coarse=coarse)
        assert np.array_equal(bits(ml.precondition(rs[2])), bits(Hv.precondition(rs[2])))
        R = np.stack([rs[2], -2.0 * rs[2], rng.standard_normal(rs[2].size)])
        Z = ml.precondition_many(R)
        for k in range(3):
            assert np.array_equal(bits(Z[k]), bits(ml.precondition(R[k])))
    # the solve with the hierarchy, and its many form
    b = rng.standard_normal((2, ops[2].fixed.size))
    u0 = np.zeros_like(b)
    X, infos = ml.solve_many(b, u0, rtol=1e-10, maxit=2000)
    for k in range(2):
        x, info = ml.solve(b[k], u0[k], rtol=1e-10, maxit=2000)
        assert info["converged"] == 1 and np.array_equal(bits(X[k]), bits(x)) and same_info(infos[k], info)
        r = ops[2].residual(b[k], x)
        assert np.sqrt(np.sum(r * r)) <= 1.01e-10 * ops[2].reference_norm(b[k], u0[k])
    ml.set_local(False)
    ml.set_coarse(False)


# ---- the flux condition of the equilibrator --------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3])
def test_robin_flux_feeds_the_equilibrator(oracle_mod, k):
    """robin_flux bits, then update_flux_bc, then equilibrate: the oracle with the same boundary_values within the
    tolerance of tests/test_inhomogeneous_bc.py, 1e-11 of the largest coefficient, on the mesh of its GPU case.  The
    right-hand side is random DG_{k-1} data, as the synthetic data of that test: the tolerance is relative to the
    result, and the rounding of an equilibration scales with its data, so the result must not lie orders of magnitude
    below the data - which it does for the smooth model problem, where u_h is nearly equilibrated already.  u_h is the
    Galerkin solution for that data (the patch problems on the Robin side are pure Neumann problems and need it)."""
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.mesh import create_unit_square
    from test_gpu_bc_update import dense_table, numpy_dofs
    mesh = create_unit_square(7, shuffle_seed=5, perturb=0.3)
    fh = np.random.default_rng(20 + k).standard_normal(mesh.ncells * k * (k + 1) // 2)
    lv = rb.galerkin_level(mesh, k, fh)
    right, u = lv["right"], lv["u"]
    dm = cpp.DeviceMesh(mesh)
    h = cpp.PrimalPoisson(dm, k)
    h.set_dirichlet(lv["dirichlet"])
    h.set_robin(right, alpha=rb.ALPHA)
    s, wq = rb.flux_rule(k)
    ue = np.random.default_rng(k).standard_normal((right.size, s.size))
    alpha = np.full(right.size, rb.ALPHA)
    assert np.array_equal(bits(h.robin_flux(u, s, ue)), bits(primal.robin_flux(mesh, k, right, alpha, u, s, ue)))
    g = h.robin_flux(u, s)
    assert np.array_equal(bits(g), bits(primal.robin_flux(mesh, k, right, alpha, u, s)))
    # (two roundings of a sum of p + 1 products with a basis that reaches 1: a few units of the last place of max |u|)
    assert np.abs(g - rb.ALPHA * rb.trace_values(mesh, k, right, u, s)).max() <= 64 * rb.U * np.abs(u).max()
    eq = cpp.SemiExplicitEquilibrator(dm, k, 1)
    eq.set_boundary(lv["ft"])
    eq.update_flux_bc(0, right, g, s, wq, vector=False)
    x = eq.equilibrate_host(lv["G"][None], fh[None])[0]
    r64 = right.astype(np.int64)
    bv = dense_table(mesh, k, 1, {0: (r64, numpy_dofs(mesh, k, r64, s, wq, g, False)[0])})
    ref = oracle_mod.se_reconstruct(mesh, k, lv["ft"], lv["G"][None], fh[None], boundary_values=bv)[0]
    print(f"k={k}: max |x - ref| / max |ref| = {np.abs(x - ref).max() / np.abs(ref).max():.2e}, max |ref| = "
          f"{np.abs(ref).max():.2e}, max |G| = {np.abs(lv['G']).max():.2e}")
    assert np.abs(x - ref).max() <= 1e-11 * np.abs(ref).max()


# ---- robin_flux at every degree and point count ------------------------------------------------------------------------
def flux_rules():
    """the point sets of the flux tests: one point at each end of the facet, four and RF_MAX_NQ = 64 points with both
    ends among them"""
    rng = np.random.default_rng(64)
    inner4, inner64 = rng.random(2), rng.random(62)
    return [np.array([0.0]), np.array([1.0]), np.concatenate([[0.0], inner4, [1.0]]),
            np.concatenate([[1.0], inner64, [0.0]])]


@pytest.mark.parametrize("name", ["bowtie", "triangle"])
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_robin_flux_bit_for_bit_at_every_degree(name, p):
    """robin_flux against primal.robin_flux at nq = 1, 4 and 64, with and without u_ext, through host memory and through
    device memory on a non-blocking stream.  `bowtie` has facets of both orientations against their cell and the pinch
    node, `triangle` every vertex in two listed facets; s = 0 and s = 1 are among the points."""
    import torch
    from dolfinx_eqlb_amd import cpp
    c = case(name, p)
    h, mesh, robin, alpha = c["h"], c["mesh"], c["robin"], c["alpha"]
    rules = flux_rules()
    assert [s.size for s in rules] == [1, 1, 4, 64]
    rng = np.random.default_rng(pm.seed_of("robin_flux", mesh.ncells, p))
    u = rng.standard_normal(c["op"].ndofs)
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)      # non-blocking: not ordered against the default stream
    torch.cuda.synchronize()
    for s in rules:
        for ue in (None, rng.standard_normal((robin.size, s.size))):
            ref = primal.robin_flux(mesh, p, robin, alpha, u, s, ue)
            assert ref.shape == (robin.size, s.size) and np.all(np.isfinite(ref))
            assert np.array_equal(bits(h.robin_flux(u, s, ue)), bits(ref))
            with torch.cuda.stream(st):
                d_u = torch.from_numpy(u).to(dev)
                d_e = None if ue is None else torch.from_numpy(ue).to(dev)
                d_o = torch.full((robin.size, s.size), float("nan"), dtype=torch.float64, device=dev)
                h.robin_flux_raw(d_u.data_ptr(), s, None if ue is None else d_e.data_ptr(), d_o.data_ptr(),
                                 cpp.MEM_DEVICE, st.cuda_stream)
            st.synchronize()
            assert np.array_equal(bits(d_o.cpu().numpy()), bits(ref))


def test_skipped_ids_of_a_device_memory_list_give_nan_rows():
    """a list in device memory with an interior facet and an id >= nfacets in its middle: those rows of the flux are
    NaN, in host and in device memory, and every other row has the bits of the statement on the list without them"""
    import torch
    from dolfinx_eqlb_amd import cpp
    p = 2
    c = case("square576", p)
    mesh, robin, alpha = c["mesh"], c["robin"], c["alpha"]
    interior = int(np.nonzero(np.diff(mesh.facet_cells_offsets) == 2)[0][0])
    at = np.array([3, 11])
    lst = np.insert(robin, at, [interior, mesh.nfacets]).astype(np.int32)       # (positions 3 and 12 of lst)
    al = np.insert(alpha, at, [2.0, 3.0])
    bad = np.zeros(lst.size, dtype=bool)
    bad[[3, 12]] = True
    assert np.array_equal(lst[~bad], robin) and lst[3] == interior and lst[12] == mesh.nfacets
    dev = torch.device("cuda:0")
    h = cpp.PrimalPoisson(c["dm"], p, c["kappa"])
    d_f, d_a = torch.from_numpy(lst).to(dev), torch.from_numpy(al).to(dev)
    torch.cuda.synchronize()
    h.set_robin_raw(lst.size, d_f.data_ptr(), 1.0, d_a.data_ptr(), cpp.MEM_DEVICE, 0)
    assert h.robin_count() == lst.size
    s = np.array([0.0, 0.25, 0.6, 1.0])
    rng = np.random.default_rng(12)
    u, ue = rng.standard_normal(c["op"].ndofs), rng.standard_normal((lst.size, s.size))
    for e in (None, ue):
        ref = primal.robin_flux(mesh, p, robin, alpha, u, s, None if e is None else e[~bad])
        d_u = torch.from_numpy(u).to(dev)
        d_e = None if e is None else torch.from_numpy(e).to(dev)
        d_o = torch.zeros((lst.size, s.size), dtype=torch.float64, device=dev)
        h.robin_flux_raw(d_u.data_ptr(), s, None if e is None else d_e.data_ptr(), d_o.data_ptr(), cpp.MEM_DEVICE, 0)
        torch.cuda.synchronize()
        for got in (d_o.cpu().numpy(), h.robin_flux(u, s, e)):
            assert np.all(np.isnan(got[bad])) and np.array_equal(bits(got[~bad]), bits(ref))


def test_a_raw_list_is_not_remembered_and_not_carried():
    """set_robin(A), then set_robin_raw(B) in device memory: the host does not know B, so robin_list() raises and does
    not return A; set_robin(C) makes it return C.  Refinement.carry_robin of a handle that was given only a raw list
    raises and leaves `new` as it was."""
    import torch
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.mesh import create_unit_square
    mesh = create_unit_square(4, shuffle_seed=3, perturb=0.15)
    dm = cpp.DeviceMesh(mesh)
    ref = dm.refine(np.arange(mesh.ncells, dtype=np.int32), keep_plan=True)
    left, bottom, right, top = rb.sides(mesh)
    A, B, C_ = right, np.concatenate([top, left]).astype(np.int32), bottom
    aA, aC = rb.alpha_of(A.size), rb.alpha_of(C_.size, seed=3)
    p = 2
    message = r"robin_list: the handle's list was not given through set_robin \(host arrays\)"
    dev = torch.device("cuda:0")
    d_B = torch.from_numpy(B).to(dev)
    torch.cuda.synchronize()

    h = cpp.PrimalPoisson(dm, p)
    assert h.robin_list()[0].size == 0 and h.robin_list()[1].shape == (0,)
    h.set_robin(A, facet_alpha=aA)
    assert np.array_equal(h.robin_list()[0], A) and np.array_equal(bits(h.robin_list()[1]), bits(aA))
    h.set_robin_raw(B.size, d_B.data_ptr(), 2.0, None, cpp.MEM_DEVICE, 0)
    assert h.robin_count() == B.size
    with pytest.raises(RuntimeError, match=message):
        h.robin_list()
    h.set_robin(C_, facet_alpha=aC)
    assert np.array_equal(h.robin_list()[0], C_) and np.array_equal(bits(h.robin_list()[1]), bits(aC))
    h.set_robin_raw(0, None, 1.0, None, cpp.MEM_DEVICE, 0)          # (an empty raw list: the term off, nothing to know)
    assert h.robin_count() == 0 and h.robin_list()[0].size == 0

    # carry_robin: `old` knows only a raw list; `new` holds a list of its own and keeps it
    old, new = cpp.PrimalPoisson(dm, p), cpp.PrimalPoisson(ref.dmesh, p)
    old.set_robin_raw(B.size, d_B.data_ptr(), 2.0, None, cpp.MEM_DEVICE, 0)
    mesh2 = ref.dmesh.mesh
    D = rb.sides(mesh2)[1]
    aD = rb.alpha_of(D.size, seed=4)
    new.set_robin(D, facet_alpha=aD)
    u = np.random.default_rng(8).standard_normal(new.ndofs)
    before = (new.apply(u), new.diagonal(), new.robin_weights())
    with pytest.raises(RuntimeError, match=message):
        ref.carry_robin(old, new)
    assert np.array_equal(new.robin_list()[0], D) and np.array_equal(bits(new.robin_list()[1]), bits(aD))
    for was, now in zip(before, (new.apply(u), new.diagonal(), new.robin_weights())):
        assert np.array_equal(bits(was), bits(now))
    op = primal.PoissonOperator(mesh2, p)
    op.set_robin(D, facet_alpha=aD)
    assert np.array_equal(bits(new.apply(u)), bits(op.apply(u)))
