"""The spring term of the P_p^2 elasticity handle on the device (cpp.PrimalElasticity.set_springs;
csrc/eqlb_primal_gather.inc, eqlb_primal_elasticity.hip, eqlb_primal_matrix.hip): the rule is the bits of the numpy
statement (dolfinx_eqlb_amd/lsolver/primal.py: ElasticityOperator.set_springs) everywhere - apply (masked and not),
diagonal, residual, spring_weights, matrix, matrix_values and csr_apply at p = 1 ... 4, alone and together with
set_shear, set_reaction and a mask that fixes one component only on part of the spring side; lists in device memory on a
non-blocking stream; hierarchies with the list carried by carry_springs on every level (BPX, local, coarse and the
factor); the solves without any Dirichlet row; spring_flux.  No tolerance appears below except where a solve is checked
against its own stopping rule.

The cases (tests/spring_cases.py: facet-wise random tensors, every fifth zero, every third rank one, the rest full):
`bowtie` (the pinched vertex lies in four spring facets), `triangle` and `right1` (every row is a spring row: no free
interior), `hole` (the inner loop only), `two_parts`, `wg256` (whole workgroups of the cell kernel), the 576-cell square
with a Dirichlet side, `sq91` at p = 1 ... 4 (33 490, 133 226, 299 210 and 531 442 rows: from p = 2 on more than the
131 072 rows of one streaming pass, so that the later passes of a block hold spring rows too), and - none of these has
a row count that ends on a chunk edge - the 7 x 8 rectangle at p = 1: 128 nodes, so 256 rows, exactly one chunk of the
sum pass and of the table that goes with it.  On `sq91` the matrix pieces are compared at p = 1, 2, 3; at p = 4 the
numpy statement of the 24 926 724 entries and of csr_apply alone takes 14 s on the host, beyond what a case of this
suite may take, and the matrix kernel runs no other path there than at p = 3 (one thread per spring DOF, whatever the
row count)."""

import numpy as np
import pytest

import elasticity_cases as ec
import primal_mesh_cases as pm
import spring_cases as sp_
from dolfinx_eqlb_amd.lsolver import primal
from spring_cases import bits

pytestmark = pytest.mark.gpu

_CACHE = {}
NAMES = ("bowtie", "triangle", "right1", "hole", "two_parts", "wg256", "square576")


def device_mesh(name):
    if ("dm", name) not in _CACHE:
        from dolfinx_eqlb_amd import cpp
        mesh, springs, K, fixed = sp_.layout(name)
        _CACHE["dm", name] = (cpp.DeviceMesh(mesh), springs, K, fixed)
    return _CACHE["dm", name]


def case(name, p, terms=False):
    """the statement and the handle of one (mesh, p), both with the spring list; terms: also a cell-wise shear modulus,
    a cell-wise reaction coefficient and a mask that fixes component 0 on the first third of the spring list and
    component 1 on its last facet only"""
    key = (name, p, terms)
    if key not in _CACHE:
        from dolfinx_eqlb_amd import cpp
        dm, springs, K, fixed = device_mesh(name)
        mesh = dm.mesh
        pi = ec.pi1_of(mesh.ncells)
        op = primal.ElasticityOperator(mesh, p, cell_pi1=pi)
        h = cpp.PrimalElasticity(dm, p, cell_pi1=pi)
        if terms:
            rng = np.random.default_rng(3)
            mu, c = 0.5 + rng.random(mesh.ncells), 3.0 * rng.random(mesh.ncells)
            fixed = (springs[:max(1, springs.size // 3)], springs[-1:])
            for o in (op, h):
                o.set_shear(cell_mu=mu)
                o.set_reaction(cell_c=c)
        for o in (op, h):
            o.set_dirichlet(*fixed)
            o.set_springs(springs, facet_k=K)
        _CACHE[key] = dict(dm=dm, mesh=mesh, op=op, h=h, springs=springs, K=K, fixed=fixed, pi=pi)
    return _CACHE[key]


def check_pieces(c, matrix=True):
    from dolfinx_eqlb_amd import cpp
    op, h, mesh = c["op"], c["h"], c["mesh"]
    n = 2 * op.ndofs
    rng = np.random.default_rng(pm.seed_of("springs", mesh.ncells, op.p))
    u, b = rng.standard_normal(n), rng.standard_normal(n)
    assert np.array_equal(bits(h.spring_weights()), bits(op.spring_weights())) and h.spring_count() == c["springs"].size
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
        if mesh.ncells > 10000:     # (the rule of `eliminate` on the values at hand: the statement's second pass costs seconds)
            rows = np.repeat(np.arange(n), np.diff(rp))
            re = np.where(op.fixed[rows] | op.fixed[rx], np.where(rows == rx, 1.0, 0.0), rv)
        else:
            re = op.matrix(eliminate=True)[2]
        assert np.array_equal(bits(h.matrix_values(eliminate=True)), bits(re))
        assert np.array_equal(bits(h.matrix_values()), bits(rv))
        assert np.array_equal(bits(cpp.csr_apply(ip, ix, v, u)), bits(primal.csr_apply(rp, rx, rv, u)))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_operator_pieces_bit_for_bit(name, p):
    c = case(name, p)
    fresh = primal.ElasticityOperator(c["mesh"], p, cell_pi1=c["pi"])
    u = np.random.default_rng(p).standard_normal(2 * fresh.ndofs)
    assert not np.array_equal(c["op"].apply(u), fresh.apply(u))       # (the term is there)
    check_pieces(c)


@pytest.mark.parametrize("name", ["bowtie", "triangle", "square576"])
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_with_shear_reaction_and_a_mask_per_component(name, p):
    c = case(name, p, terms=True)
    fx = c["op"].fixed.reshape(-1, 2)
    assert np.any(fx[:, 0] & ~fx[:, 1])           # rows with one component fixed only: only_fixed per component
    check_pieces(c)


def test_a_row_count_on_a_chunk_edge():
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.mesh import create_rectangle
    mesh = create_rectangle(7, 8, shuffle_seed=3, perturb=0.15)
    springs = mesh.boundary_facets().astype(np.int32)
    K = sp_.tensors_of(mesh, springs)
    op = primal.ElasticityOperator(mesh, 1)
    assert 2 * op.ndofs == 256
    h = cpp.PrimalElasticity(cpp.DeviceMesh(mesh), 1)
    for o in (op, h):
        o.set_springs(springs, facet_k=K)
    check_pieces(dict(op=op, h=h, mesh=mesh, springs=springs))


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_more_rows_than_one_pass(p):
    """`sq91`, springs on the whole boundary in a shuffled order, component 0 fixed on forty of the facets and component
    1 on seven; the matrix pieces at p <= 3 (the head of this file)"""
    from dolfinx_eqlb_amd import cpp
    if "sq91" not in _CACHE:
        mesh = pm.mesh_of("sq91")
        springs = mesh.boundary_facets().astype(np.int32)
        springs = springs[np.random.default_rng(5).permutation(springs.size)]
        _CACHE["sq91"] = (cpp.DeviceMesh(mesh), springs, sp_.tensors_of(mesh, springs))
    dm, springs, K = _CACHE["sq91"]
    mesh = dm.mesh
    op = primal.ElasticityOperator(mesh, p)
    assert (2 * op.ndofs > pm.ROWS_PER_PASS) == (p >= 2)
    h = cpp.PrimalElasticity(dm, p)
    for o in (op, h):
        o.set_dirichlet(springs[:40], springs[-7:])
        o.set_springs(springs, facet_k=K)
    if p >= 2:      # spring rows beyond the first pass: the facet DOFs are numbered behind the 16 745 vertices
        assert 2 * primal.facet_dofs(mesh, p, springs).max() >= pm.ROWS_PER_PASS
    check_pieces(dict(op=op, h=h, mesh=mesh, springs=springs), matrix=p <= 3)
    h.close()


@pytest.mark.parametrize("name", ["square576", "bowtie"])
@pytest.mark.parametrize("p", [1, 3])
def test_empty_list_is_a_fresh_handle_and_a_new_list_replaces_the_old(name, p):
    from dolfinx_eqlb_amd import cpp
    c = case(name, p)
    mesh, springs, K = c["mesh"], c["springs"], c["K"]
    op, fresh = (primal.ElasticityOperator(mesh, p, cell_pi1=c["pi"]) for _ in range(2))
    h = cpp.PrimalElasticity(c["dm"], p, cell_pi1=c["pi"])
    never = cpp.PrimalElasticity(c["dm"], p, cell_pi1=c["pi"])
    u = np.random.default_rng(2).standard_normal(2 * op.ndofs)
    for o in (op, h):
        o.set_springs(springs[:5], k=3.0)
    assert np.array_equal(bits(h.apply(u)), bits(op.apply(u))) and h.spring_count() == 5
    for o in (op, h):
        o.set_springs(springs[3:], facet_k=K[3:])
    y, d = h.apply(u), h.diagonal()
    assert np.array_equal(bits(y), bits(op.apply(u))) and np.array_equal(bits(d), bits(op.diagonal()))
    h.set_springs(springs[3:], facet_k=K[3:])                        # two identical calls: identical bits
    assert np.array_equal(bits(h.apply(u)), bits(y)) and np.array_equal(bits(h.diagonal()), bits(d))
    h.set_springs([])
    assert np.array_equal(bits(h.apply(u)), bits(never.apply(u))) and np.array_equal(bits(h.apply(u)), bits(fresh.apply(u)))
    assert np.array_equal(bits(h.diagonal()), bits(never.diagonal())) and h.spring_count() == 0
    assert h.spring_weights().shape == (0, 3)
    # rank one everywhere: the term is on and makes nothing definite; so does k = 0
    for kw in (dict(facet_k=primal.spring_tensor(mesh, springs, 4.0)), dict(k=0.0)):
        h.set_springs(springs, **kw)
        with pytest.raises(RuntimeError, match="singular: component 0 has no Dirichlet DOF"):
            h.solve(u, np.zeros_like(u))
    h.set_springs([])
    with pytest.raises(RuntimeError, match="singular: component 0 has no Dirichlet DOF"):
        h.solve(u, np.zeros_like(u))
    with pytest.raises(RuntimeError, match="no spring term"):
        h.spring_flux(u, [0.5])


def test_refusals_in_host_memory_leave_the_handle_as_it_was():
    c = case("square576", 2)
    h, op, mesh, springs, K = c["h"], c["op"], c["mesh"], c["springs"], c["K"]
    u = np.random.default_rng(1).standard_normal(2 * op.ndofs)
    interior = int(np.nonzero(np.diff(mesh.facet_cells_offsets) == 2)[0][0])
    for bad in (interior, -1, mesh.nfacets):
        lst = springs.copy()
        lst[4] = bad
        with pytest.raises(RuntimeError, match=r"facets\[4\] = %d is no boundary facet" % bad):
            h.set_springs(lst, facet_k=K)
    lst = springs.copy()
    lst[7] = lst[2]
    with pytest.raises(RuntimeError, match=r"facets\[7\] = %d is listed twice" % lst[2]):
        h.set_springs(lst, facet_k=K)
    for col in range(3):
        for value in (np.nan, np.inf, -np.inf):
            k = K.copy()
            k[3, col] = value
            with pytest.raises(RuntimeError, match=r"facet_k\[3\] = .* is not finite"):
                h.set_springs(springs, facet_k=k)
    k = K.copy()
    k[3] = (-1.0, 0.0, 2.0)
    with pytest.raises(RuntimeError, match=r"facet_k\[3\]: k00 = -1 is negative"):
        h.set_springs(springs, facet_k=k)
    k[3] = (2.0, 0.0, -0.5)
    with pytest.raises(RuntimeError, match=r"facet_k\[3\]: k11 = -0.5 is negative"):
        h.set_springs(springs, facet_k=k)
    k[3] = (1.0, 1.0 + 1e-14, 1.0)
    with pytest.raises(RuntimeError, match=r"facet_k\[3\] = .* is not positive semidefinite"):
        h.set_springs(springs, facet_k=k)
    k[2] = (np.nan, 0.0, 1.0)                                     # by facet, in the order of the list
    with pytest.raises(RuntimeError, match=r"facet_k\[2\] = .* is not finite"):
        h.set_springs(springs, facet_k=k)
    lst = springs.copy()
    lst[1] = interior
    with pytest.raises(RuntimeError, match=r"facets\[1\] = %d is no boundary facet" % interior):
        h.set_springs(lst, facet_k=k)
    for value in (-1.0, np.nan, np.inf):
        with pytest.raises(RuntimeError, match="k = .* is negative, NaN or infinite"):
            h.set_springs(springs, k=value)
    assert np.array_equal(bits(h.apply(u)), bits(op.apply(u))) and np.array_equal(bits(h.diagonal()), bits(op.diagonal()))
    assert np.array_equal(bits(h.spring_weights()), bits(op.spring_weights()))
    # the edge of the allowance passes on the device as on the host
    k = K.copy()
    k[3] = (1.0, 1.0 + 2.0 ** -52, 1.0)
    fresh = type(h)(c["dm"], 2, cell_pi1=c["pi"])
    fresh.set_springs(springs, facet_k=k)
    ref = primal.ElasticityOperator(mesh, 2, cell_pi1=c["pi"])
    ref.set_springs(springs, facet_k=k)
    assert np.array_equal(bits(fresh.apply(u)), bits(ref.apply(u)))


# ---- lists in device memory, a non-blocking stream, spring_flux --------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_device_memory_list_and_spring_flux_on_a_non_blocking_stream(p):
    import torch
    from dolfinx_eqlb_amd import cpp
    c = case("square576", p)
    op, mesh, springs, K = c["op"], c["mesh"], c["springs"], c["K"]
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)      # non-blocking: not ordered against the default stream
    h = cpp.PrimalElasticity(c["dm"], p, cell_pi1=c["pi"])
    h.set_dirichlet(*c["fixed"])
    torch.cuda.synchronize()
    interior = int(np.nonzero(np.diff(mesh.facet_cells_offsets) == 2)[0][0])
    # ids that are no boundary facet are skipped in device memory: nothing is read out of range, the rest is taken
    lst = np.concatenate([springs, [-7, mesh.nfacets + 3, interior]]).astype(np.int32)
    kk = np.concatenate([K, [[1.0, 0.0, 1.0], [2.0, 0.5, 2.0], [3.0, 0.0, 1.0]]])
    n = springs.size
    u = np.random.default_rng(p).standard_normal(2 * op.ndofs)
    rules = {nq: np.random.default_rng(nq).random(nq) for nq in (1, 4, 64)}
    rules[4][:2] = (0.0, 1.0)
    ue = {nq: np.random.default_rng(nq + p).standard_normal((2, lst.size, nq)) for nq in rules}
    with torch.cuda.stream(st):
        d_f, d_k = torch.from_numpy(lst).to(dev), torch.from_numpy(kk).to(dev)
        d_u = torch.from_numpy(u).to(dev)
        d_y = torch.full_like(d_u, float("nan"))
        d_w = torch.full((lst.size, 3), float("nan"), dtype=torch.float64, device=dev)
        h.set_springs_raw(lst.size, d_f.data_ptr(), 1.0, d_k.data_ptr(), cpp.MEM_DEVICE, st.cuda_stream)
        h.apply_raw(d_u.data_ptr(), d_y.data_ptr(), False, cpp.MEM_DEVICE, st.cuda_stream)
        assert h.spring_weights_raw(d_w.data_ptr(), lst.size, cpp.MEM_DEVICE, st.cuda_stream) == lst.size
        d_out = {}
        for nq, s in rules.items():
            d_e = torch.from_numpy(ue[nq]).to(dev)
            d_out[nq, True] = torch.full((2, lst.size, nq), 7.0, dtype=torch.float64, device=dev)
            d_out[nq, False] = torch.full((2, lst.size, nq), 7.0, dtype=torch.float64, device=dev)
            h.spring_flux_raw(d_u.data_ptr(), s, d_e.data_ptr(), d_out[nq, True].data_ptr(), cpp.MEM_DEVICE, st.cuda_stream)
            h.spring_flux_raw(d_u.data_ptr(), s, None, d_out[nq, False].data_ptr(), cpp.MEM_DEVICE, st.cuda_stream)
    st.synchronize()
    assert np.array_equal(bits(d_y.cpu().numpy()), bits(op.apply(u)))
    w = d_w.cpu().numpy()
    assert np.array_equal(bits(w[:n]), bits(op.spring_weights())) and not np.any(w[n:])
    for nq, s in rules.items():
        for with_ext in (True, False):
            e = ue[nq] if with_ext else None
            ref = primal.spring_flux(mesh, p, springs, K, u, s, None if e is None else e[:, :n])
            got = d_out[nq, with_ext].cpu().numpy()
            assert np.array_equal(bits(got[:, :n]), bits(ref)), (nq, with_ext)
            assert np.all(np.isnan(got[:, n:]))                      # a facet the list skipped
            host = h.spring_flux(u, s, e)                            # host memory: the same bits
            assert np.array_equal(bits(host[:, :n]), bits(ref)) and np.all(np.isnan(host[:, n:]))
    with pytest.raises(RuntimeError, match="not given through set_springs"):
        h.spring_list()                                              # (a list in device memory: carry_springs refuses it)
    # the handle of the cases (host memory list) gives the statement too, in the order of ITS list
    s = rules[4]
    assert np.array_equal(bits(c["h"].spring_flux(u, s, ue[4][:, :n])),
                          bits(primal.spring_flux(mesh, p, springs, K, u, s, ue[4][:, :n])))
    for bad in ([], np.zeros(65), [1.5]):
        with pytest.raises(RuntimeError, match="nq = |outside"):
            c["h"].spring_flux(u, bad)


# ---- hierarchies with springs on every level -------------------------------------------------------------------------------
def spring_hierarchy(name, p):
    """the levels of primal_mesh_cases.levels_of(name) refined on the device, springs on the whole boundary of level 0
    and carried by carry_springs, no Dirichlet row anywhere"""
    key = ("hier", name, p)
    if key not in _CACHE:
        from dolfinx_eqlb_amd import cpp
        from dolfinx_eqlb_amd.mesh import refine
        from test_gpu_primal_meshes import device_levels
        dms, refs = device_levels(name)
        meshes = [d.mesh for d in dms]
        links = [(r.parent_cell, r.node_parent_facet) for r in refs]
        coeff = pm.mc.coefficients(meshes, links, ec.pi1_of)
        ops, hs, lists = [], [], []
        f = K = None
        for l, (dm, m, pi) in enumerate(zip(dms, meshes, coeff)):
            op, h = primal.ElasticityOperator(m, p, cell_pi1=pi), cpp.PrimalElasticity(dm, p, cell_pi1=pi)
            if l == 0:
                f = m.boundary_facets().astype(np.int32)
                f = f[np.random.default_rng(1).permutation(f.size)]
                K = sp_.tensors_of(m, f)
                h.set_springs(f, facet_k=K)
            else:
                f2, K2 = refs[l - 1].carry_springs(hs[-1], h)
                rf, rK = refine.carry_springs_list(meshes[l - 1], refs[l - 1].node_parent_facet, m, f, K)
                assert np.array_equal(f2, rf) and np.array_equal(bits(K2), bits(rK)) and f2.size >= f.size
                assert np.array_equal(h.spring_list()[0], f2) and np.array_equal(bits(h.spring_list()[1]), bits(K2))
                f, K = f2, K2
            op.set_springs(f, facet_k=K)
            assert np.array_equal(bits(h.spring_weights()), bits(op.spring_weights()))
            assert np.all(np.diff(m.facet_cells_offsets)[f] == 1) and np.unique(f).size == f.size
            ops.append(op)
            hs.append(h)
            lists.append((f, K))
        assert lists[-1][0].size > lists[0][0].size
        _CACHE[key] = dict(hs=hs, ops=ops, refs=refs, lists=lists)
    return _CACHE[key]


@pytest.mark.parametrize("name,p", [("sq6_two", 1), ("sq6_two", 2), ("disk70", 1), ("disk70", 2)])
def test_hierarchy_precondition_factor_and_solve_bit_for_bit(name, p):
    """carry_springs after one (sq6_two) and two (disk70) refinements is checked where the hierarchy is built"""
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.lsolver import Hierarchy
    from test_gpu_multilevel_coarse import same_factor
    c = spring_hierarchy(name, p)
    ops, hs, refs = c["ops"], c["hs"], c["refs"]
    assert not any(op.fixed.any() for op in ops) and ops[0].spring_positive()
    n = ops[-1].fixed.size
    rng = np.random.default_rng(pm.seed_of("spring-hier", name, p))
    r = rng.standard_normal(n)
    ml = cpp.Multilevel(hs, refs)
    for local, coarse in ((False, False), (True, False), (False, True), (True, True)):
        ml.set_local(local)
        ml.set_coarse(coarse)
        H = Hierarchy(ops, refs, local=local, coarse=coarse)
        assert np.array_equal(bits(ml.precondition(r)), bits(H.precondition(r))), (local, coarse)
        if coarse and not local:
            same_factor(ml, H)
            assert ml.coarse_rows == ops[0].fixed.size               # no Dirichlet row: every row of level 0
    # the restriction carries no spring term: the bits of a hierarchy whose levels never had one
    plain = [primal.ElasticityOperator(o.mesh, p, cell_pi1=o.pi) for o in ops]
    for level in range(len(ops) - 2, -1, -1):
        v = rng.standard_normal(ops[level + 1].fixed.size)
        assert np.array_equal(bits(ml.restrict(level, v)), bits(Hierarchy(plain, refs).restrict(level, v)))
    # the solves without any Dirichlet row: the Jacobi one of the finest handle, and the hierarchy's
    b = rng.standard_normal(n)
    op = ops[-1]
    tol = 1e-10 * op.reference_norm(b, np.zeros(n))
    u, info = hs[-1].solve(b, np.zeros(n), rtol=1e-10, maxit=20000)
    assert info["converged"] == 1 and info["breakdown"] == 0
    rs = op.residual(b, u)
    assert np.sqrt(np.sum(rs * rs)) <= 1.01 * tol
    ml.set_local(True)
    ml.set_coarse(True)
    u2, info2 = ml.solve(b, np.zeros(n), rtol=1e-10, maxit=2000)
    assert info2["converged"] == 1 and info2["breakdown"] == 0 and info2["iterations"] < info["iterations"]
    rs = op.residual(b, u2)
    assert np.sqrt(np.sum(rs * rs)) <= 1.01 * tol
    # a change on level 0: the factor is a snapshot until set_coarse is called again
    f0, K0 = c["lists"][0]
    hs[0].set_springs(f0, facet_k=2.0 * K0)
    ops0 = primal.ElasticityOperator(ops[0].mesh, p, cell_pi1=ops[0].pi)
    ops0.set_springs(f0, facet_k=2.0 * K0)
    ml.set_local(False)
    ml.set_coarse(True)
    assert np.array_equal(bits(ml.precondition(r)), bits(Hierarchy([ops0] + ops[1:], refs, coarse=True).precondition(r)))
    hs[0].set_springs(f0, facet_k=K0)
    ml.close()
