"""The cell-wise shear modulus of the elasticity solve on the device (eqlb_elasticity_set_shear) and of the projected
stress (eqlb_primal_stress_dg_mu) against their statements, bit for bit - there is no tolerance anywhere in this file.

  operator   apply (masked and raw), diagonal and residual of cpp.PrimalElasticity after set_shear give the bits of
             lsolver.primal.ElasticityOperator after set_shear: y_loc = mu_T v, with a reaction term (mu_T v) + wm m
  stress     cpp.primal_stress_dg(mu / cell_mu) gives mu_T times the values of the call without the keywords, rounded once
             (the statement of the entry: one product on top of the value formed without the term)
on meshes of tests/primal_mesh_cases.py: one and two cells, whole workgroups of the 128-cell kernel (wg128, wg256), a
partial last workgroup (delaunay), more rows than one streaming pass (sq91), det ~ 1e-14 (tiny_far) and an aspect ratio
of 1000.  Then the exact scaling by a power of two, switching the term off, the solve, the multilevel preconditioner with
the coefficient carried by Refinement.prolong_dg, the refusals and the pybind module.  Every handle here is made for its
test: a modulus left on a shared one would change the tests of other files."""

import ctypes as C

import numpy as np
import pytest

import primal_mesh_cases as pm
import reaction_cases as rc
from test_gpu_multilevel_coarse import same_factor
from test_gpu_primal_meshes import device_levels, device_mesh, make_handle
from test_gpu_primal_solve import bits

pytestmark = pytest.mark.gpu

MESHES = ("triangle", "right1", "wg128", "wg256", "delaunay", "sq91", "aspect1000", "tiny_far")
RTOL = 1e-10


def mu_of(ncells, seed=41):
    """cell-wise mu: log-uniform in [1e-3, 1e3]"""
    return 10.0 ** (-3.0 + 6.0 * np.random.default_rng(seed).random(ncells))


def case(name, p):
    """the statement, a handle of its own and the vectors of one (mesh, p), Dirichlet all around"""
    mesh = pm.mesh_of(name)
    op, coeff, args = pm.statement("elasticity", mesh, p, "all")
    h = make_handle("elasticity", device_mesh(name), p, coeff, args)
    assert h.ndofs == op.ndofs
    n = op.fixed.size
    c = dict(op=op, h=h, n=n, mesh=mesh, coeff=coeff, args=args, **pm.vectors("elasticity", mesh, p, n, name))
    c["b"] = op.load(c["d"], c["f"], c["e"])     # (the load knows no shear modulus)
    return c


def check(c):
    """apply (raw and masked), diagonal, residual and the unchanged load of the handle against the statement"""
    op, h, u, b = c["op"], c["h"], c["u"], c["b"]
    assert np.array_equal(bits(h.apply(u)), bits(op.apply(u)))
    assert np.array_equal(bits(h.apply(u, masked=True)), bits(op.apply(u, masked=True)))
    assert np.array_equal(bits(h.diagonal()), bits(op.diagonal()))
    assert np.array_equal(bits(h.residual(b, u)), bits(op.residual(b, u)))
    assert np.array_equal(bits(h.load(c["d"], c["f"], c["e"])), bits(b))


# ---- 1. the operator, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_shear_bit_for_bit(name, p):
    c = case(name, p)
    op, h, ncells = c["op"], c["h"], c["mesh"].ncells
    if name == "sq91" and p >= 2:
        assert c["n"] > pm.ROWS_PER_PASS
    plain = op.apply(c["u"])
    mu = mu_of(ncells)
    assert mu.min() >= 1e-3 and mu.max() <= 1e3
    op.set_shear(cell_mu=mu)
    h.set_shear(cell_mu=mu)
    check(c)
    assert not np.array_equal(op.apply(c["u"]), plain)
    # once more with a cell-wise reaction coefficient at the same time: (mu_T v) + wm m
    cc = rc.c_of(ncells)
    op.set_reaction(cell_c=cc)
    h.set_reaction(cell_c=cc)
    check(c)
    # the reaction term off again, the modulus stays
    op.set_reaction()
    h.set_reaction()
    check(c)


def test_shear_in_device_memory_is_copied():
    import torch
    c = case("delaunay", 3)
    op, h, n = c["op"], c["h"], c["n"]
    mu = mu_of(c["mesh"].ncells, seed=43)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    u, mm = t(c["u"]), t(mu)
    out = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    op.set_shear(cell_mu=mu)
    h.set_shear_raw(1.0, mm.data_ptr())
    h.apply_raw(u.data_ptr(), out.data_ptr(), False)
    assert np.array_equal(bits(out.cpu().numpy()), bits(op.apply(c["u"])))
    h.diagonal_raw(out.data_ptr())
    assert np.array_equal(bits(out.cpu().numpy()), bits(op.diagonal()))
    assert np.array_equal(bits(mm.cpu().numpy()), bits(mu))      # the input is not touched
    mm.fill_(float("nan"))                                       # ... and was copied
    torch.cuda.synchronize()
    h.apply_raw(u.data_ptr(), out.data_ptr(), True)
    assert np.array_equal(bits(out.cpu().numpy()), bits(op.apply(c["u"], masked=True)))


# ---- 2. scaling, switching, solves -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 4])
def test_power_of_two_scales_exactly_and_one_restores_the_bits(p):
    c = case("wg256", p)
    h, u, b = c["h"], c["u"], c["b"]
    y0, ym0, d0, r0 = h.apply(u), h.apply(u, masked=True), h.diagonal(), h.residual(b, u)
    h.set_shear(4.0)
    assert np.array_equal(bits(h.apply(u)), bits(4.0 * y0))
    assert np.array_equal(bits(h.apply(u, masked=True)), bits(4.0 * ym0))
    assert np.array_equal(bits(h.diagonal()), bits(4.0 * d0))
    h.set_shear(cell_mu=np.full(c["mesh"].ncells, 4.0))        # the array gives what the scalar gives
    assert np.array_equal(bits(h.apply(u)), bits(4.0 * y0)) and np.array_equal(bits(h.diagonal()), bits(4.0 * d0))
    h.set_shear(1.0)                                           # off: the handle is as created
    assert np.array_equal(bits(h.apply(u)), bits(y0)) and np.array_equal(bits(h.apply(u, masked=True)), bits(ym0))
    assert np.array_equal(bits(h.diagonal()), bits(d0)) and np.array_equal(bits(h.residual(b, u)), bits(r0))
    h.set_shear(cell_mu=mu_of(c["mesh"].ncells))
    h.set_shear()                                              # the defaults switch the term off
    assert np.array_equal(bits(h.apply(u)), bits(y0)) and np.array_equal(bits(h.diagonal()), bits(d0))


@pytest.mark.parametrize("p", [1, 3])
def test_two_solves_give_the_same_bits(p):
    c = case("wg256", p)
    op, h = c["op"], c["h"]
    mu = mu_of(c["mesh"].ncells)
    op.set_shear(cell_mu=mu)
    h.set_shear(cell_mu=mu)
    b, u0, start = pm.solve_data(op, "elasticity", "shear-wg256", p, inhomogeneous=True)
    u, info = h.solve(b, start, rtol=RTOL, maxit=20000)
    u2, info2 = h.solve(b, start, rtol=RTOL, maxit=20000)
    assert info["converged"] == 1 and info["breakdown"] == 0
    assert np.array_equal(bits(u), bits(u2)) and info == info2
    rs = op.residual(b, u)                                     # the statement's residual, with the modulus
    n = op.fixed.size
    assert np.sqrt(np.sum(rs * rs)) <= RTOL * op.reference_norm(b, u0) * (1.0 + n * rc.U)
    assert np.array_equal(bits(u[op.fixed]), bits(u0[op.fixed]))


# ---- 3. the hierarchy ------------------------------------------------------------------------------------------------------
FORMS = [dict(), dict(local=True), dict(coarse=True), dict(local=True, coarse=True)]


@pytest.mark.parametrize("name,p", [("disk70", 1), ("disk70", 2), ("lshape_graded", 1)])
def test_hierarchy_with_a_shear_modulus_carried_by_prolong_dg(name, p):
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.lsolver.multilevel import Hierarchy
    dms, refs = device_levels(name)
    meshes = [d.mesh for d in dms]
    links = [(r.parent_cell, r.node_parent_facet) for r in refs]
    coeff = pm.mc.coefficients(meshes, links, pm.ec.pi1_of)
    mus = [mu_of(meshes[0].ncells, seed=47)]
    for l, ref in enumerate(refs):                             # a DG_0 coefficient crosses a refinement on the device
        mus.append(ref.prolong_dg(0, mus[-1]).ravel())
        assert np.array_equal(mus[-1], mus[l][ref.parent_cell])
    ops, hs = [], []
    for dm, m, k, mu in zip(dms, meshes, coeff, mus):
        op, _, args = pm.statement("elasticity", m, p, "all", k)
        h = make_handle("elasticity", dm, p, k, args)
        op.set_shear(cell_mu=mu)
        h.set_shear(cell_mu=mu)
        ops.append(op)
        hs.append(h)
    r = np.random.default_rng(pm.seed_of("shear-hierarchy", name, p)).standard_normal(ops[-1].fixed.size)
    for form in FORMS:
        H = Hierarchy(ops, refs, **form)
        ml = cpp.Multilevel(hs, refs, **form)
        for call in range(2):
            z = ml.precondition(r)
            assert np.array_equal(bits(z), bits(H.precondition(r))), form
        if form.get("coarse"):
            same_factor(ml, H)                                 # coarse_factor(), bit for bit
        ml.close()
    # a change on level 0 needs set_coarse(True) again: then factor and preconditioner are the statement's
    ml = cpp.Multilevel(hs, refs, coarse=True)
    ops[0].set_shear(2.0)
    hs[0].set_shear(2.0)
    ml.set_coarse(True)
    Hn = Hierarchy(ops, refs, coarse=True)
    same_factor(ml, Hn)
    assert np.array_equal(bits(ml.precondition(r)), bits(Hn.precondition(r)))
    ml.close()


# ---- 4. the projected stress -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_stress_is_mu_times_the_stress_without_it(name, p):
    from dolfinx_eqlb_amd import cpp
    mesh, dm = pm.mesh_of(name), device_mesh(name)
    cd, ndofs = dm.lagrange_dofmap(p)
    rng = np.random.default_rng(pm.seed_of("shear-stress", name, p))
    u = rng.standard_normal(2 * ndofs)
    pi1, mu = pm.ec.pi1_of(mesh.ncells), mu_of(mesh.ncells, seed=53)
    for d in sorted({p - 1, 0}):
        nd2 = (d + 1) * (d + 2)
        for kw in (dict(cell_pi1=pi1), dict(pi_1=2.5)):
            plain = cpp.primal_stress_dg(dm, p, d, cd, u, **kw)
            ref = (np.repeat(mu, nd2)[None, :] * plain)
            got = cpp.primal_stress_dg(dm, p, d, cd, u, cell_mu=mu, **kw)
            assert np.array_equal(bits(got), bits(ref)), (d, kw.keys())
            assert np.array_equal(bits(cpp.primal_stress_dg(dm, p, d, cd, u, mu=4.0, **kw)), bits(4.0 * plain))
            assert np.array_equal(bits(cpp.primal_stress_dg(dm, p, d, cd, u, mu=0.3, **kw)), bits(0.3 * plain))
            # mu = 1 and no array through the new entry: the kernel and the bits of eqlb_primal_stress_dg
            out = np.full_like(plain, np.nan)
            kc = kw.get("cell_pi1")
            cd32, uu = np.ascontiguousarray(cd, dtype=np.int32), np.ascontiguousarray(u)
            cpp.primal_stress_dg_mu_raw(dm, p, d, cd32.ctypes.data, ndofs, uu.ctypes.data, kw.get("pi_1", 1.0),
                                        None if kc is None else kc.ctypes.data, 1.0, None, out.ctypes.data, None,
                                        cpp.MEM_HOST)
            assert np.array_equal(bits(out), bits(plain))


def test_local_projection_takes_the_modulus():
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.lsolver import PrimalStress, local_projection
    mesh, dm, p = pm.mesh_of("delaunay"), device_mesh("delaunay"), 2
    cd, ndofs = dm.lagrange_dofmap(p)
    u = np.random.default_rng(3).standard_normal((ndofs, 2))
    mu = mu_of(mesh.ncells)
    ref = cpp.primal_stress_dg(dm, p, 1, cd, u, 2.0, cell_mu=mu)
    rows = local_projection(dm, 1, [PrimalStress(u, cd, p, 2.0, r, cell_mu=mu) for r in range(2)], bs=2)
    assert np.array_equal(bits(np.stack(rows)), bits(ref))
    rows = local_projection(dm, 1, [PrimalStress(u, cd, p, 2.0, r) for r in range(2)], bs=2)
    assert np.array_equal(bits(np.stack(rows)), bits(cpp.primal_stress_dg(dm, p, 1, cd, u, 2.0)))


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_cell_or_the_argument_and_the_next_call_works():
    from dolfinx_eqlb_amd import cpp
    c = case("wg128", 2)
    op, h, u, ncells = c["op"], c["h"], c["u"], c["mesh"].ncells
    op.set_shear(3.0)
    h.set_shear(3.0)
    y3, d3 = op.apply(u), op.diagonal()
    who = "eqlb_elasticity_set_shear"
    for value, where in ((0.0, 3), (-1.0, 5), (float("nan"), 0), (float("inf"), ncells - 1)):
        bad = np.ones(ncells)
        bad[where] = value
        with pytest.raises(RuntimeError, match=who + r": cell_mu\[%d\] = " % where):
            h.set_shear(cell_mu=bad)
        with pytest.raises(RuntimeError, match=who + ": mu = "):
            h.set_shear(value)
        assert np.array_equal(bits(h.apply(u)), bits(y3)) and np.array_equal(bits(h.diagonal()), bits(d3))
    with pytest.raises(RuntimeError, match="Input sizes does not match"):
        h.set_shear(cell_mu=np.ones(ncells + 1))
    L = cpp.lib()
    one = np.ones(ncells)
    assert L.eqlb_elasticity_set_shear(None, C.c_double(2.0), None, C.c_int32(cpp.MEM_HOST), None) != 0
    assert who in L.eqlb_last_error().decode() and "null handle" in L.eqlb_last_error().decode()
    assert L.eqlb_elasticity_set_shear(h._h, C.c_double(2.0), C.c_void_p(one.ctypes.data), C.c_int32(7), None) != 0
    assert who in L.eqlb_last_error().decode() and "memory space" in L.eqlb_last_error().decode()
    assert np.array_equal(bits(h.apply(u)), bits(y3)) and np.array_equal(bits(h.diagonal()), bits(d3))
    mu = mu_of(ncells)                                         # the next valid call works
    op.set_shear(cell_mu=mu)
    h.set_shear(cell_mu=mu)
    check(c)
    # the stress entry refuses the same values, the cell named
    dm = device_mesh("wg128")
    cd, ndofs = dm.lagrange_dofmap(2)
    for value in (0.0, -2.0, float("nan"), float("inf")):
        bad = np.ones(ncells)
        bad[9] = value
        with pytest.raises(RuntimeError, match=r"eqlb_primal_stress_dg_mu: cell_mu\[9\] = "):
            cpp.primal_stress_dg(dm, 2, 1, cd, u, cell_mu=bad)
        with pytest.raises(RuntimeError, match="eqlb_primal_stress_dg_mu: mu = "):
            cpp.primal_stress_dg(dm, 2, 1, cd, u, mu=value)
    with pytest.raises(RuntimeError, match="Input sizes does not match"):
        cpp.primal_stress_dg(dm, 2, 1, cd, u, cell_mu=np.ones(ncells - 1))
    assert cpp.primal_stress_dg(dm, 2, 1, cd, u, cell_mu=mu).shape == (2, ncells * 6)


def test_pybind_module_sets_and_clears_the_modulus():
    """_cpp.PrimalElasticity.set_shear: the same bits as the statement"""
    from dolfinx_eqlb_amd.eqlb import _adapter
    cm = _adapter.module()
    c = case("wg128", 2)
    op, u, mesh = c["op"], c["u"], c["mesh"]
    h = cm.PrimalElasticity(_adapter.cpp_mesh(mesh), 2, 1.0, c["coeff"])
    h.set_dirichlet(*c["args"])
    plain = op.apply(u, masked=True)
    for kw in (dict(mu=0.5), dict(cell_mu=mu_of(mesh.ncells)), dict()):
        op.set_shear(**kw)
        h.set_shear(**kw)
        assert np.array_equal(bits(h.apply(u, True)), bits(op.apply(u, masked=True)))
        assert np.array_equal(bits(h.diagonal()), bits(op.diagonal()))
    assert np.array_equal(bits(h.apply(u, True)), bits(plain))
