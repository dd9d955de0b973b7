"""Solves with a reaction term on the device: the Jacobi-preconditioned CG of cpp.PrimalPoisson / cpp.PrimalElasticity
against the assembled stiffness + mass (tests/reaction_cases.py) with the assertions of check_solution of
tests/test_gpu_primal_solve.py / tests/test_gpu_primal_elasticity.py, the iteration count against the statement's pcg,
and the multilevel preconditioner (cpp.Multilevel) with the reaction set on every level against its numpy statement
(lsolver.multilevel.Hierarchy), which works through apply and diagonal and needed no change.

c = 1 / tau is the coefficient of an implicit heat step: tau = 1 leaves the problem as stiff as without the term,
tau = 1e-4 makes the mass term dominate (c h^2 ~ 10 ... 100 on these meshes).  The cell-wise case is
reaction_cases.c_of: log-uniform in [1e-2, 1e4] with every seventh cell 0."""

import numpy as np
import pytest

import galerkin as gk
import primal_cases as pc
import primal_mesh_cases as pm
import reaction_cases as rc
from dolfinx_eqlb_amd.lsolver import primal
from test_gpu_multilevel_coarse import same_factor
from test_gpu_primal_elasticity import check_solution as check_elasticity
from test_gpu_primal_meshes import device_levels, make_handle
from test_gpu_primal_solve import bits, check_solution as check_poisson, setup

pytestmark = pytest.mark.gpu

RTOL = 1e-10
KINDS = ["tau1", "tau1e-4", "cell"]


def reaction_of(kind, ncells):
    """(the keywords of set_reaction, c_T [ncells])"""
    if kind == "cell":
        cc = rc.c_of(ncells)
        return dict(cell_c=cc), cc
    c = {"tau1": 1.0, "tau1e-4": 1e4}[kind]
    return dict(c=c), np.full(ncells, c)


def pair(dm, mesh, p, kappa, facets, kind):
    """the statement and a handle of its own with the mask and the reaction set"""
    from dolfinx_eqlb_amd import cpp
    kw, cvec = reaction_of(kind, mesh.ncells)
    op = primal.PoissonOperator(mesh, p, kappa)
    h = cpp.PrimalPoisson(dm, p, kappa)
    for x in (op, h):
        x.set_dirichlet(facets)
        x.set_reaction(**kw)
    return op, h, cvec


def solve_and_check(op, h, A, b, u0, start):
    u, info = h.solve(b, start, rtol=RTOL, maxit=5000)
    check_poisson(op, A, b, u0, u, info, RTOL)
    # the statement's PCG takes the same number of iterations up to the rounding of the inner products
    _, si = op.pcg(b, start, rtol=RTOL, maxit=5000)
    print(f"statement: {si['iterations']} iterations")
    assert abs(si["iterations"] - info["iterations"]) <= max(2, info["iterations"] // 20)
    u2, info2 = h.solve(b, start, rtol=RTOL, maxit=5000)
    assert np.array_equal(bits(u), bits(u2)) and info == info2      # two solves give the same bits
    return info


# ---- 4. the solve ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["base", "refined"])
@pytest.mark.parametrize("p", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", KINDS)
def test_solve_dirichlet_all_around(which, p, kind):
    dm, mesh = setup(which)
    kappa = pc.kappa_of(mesh.ncells)
    op, h, cvec = pair(dm, mesh, p, kappa, mesh.boundary_facets(), kind)
    d = min(p, 3)
    f = np.random.default_rng(17 * p + len(which)).standard_normal(mesh.ncells * (d + 1) * (d + 2) // 2)
    b = h.load(d, f)
    assert np.array_equal(bits(b), bits(op.load(d, f)))
    u0 = np.zeros(op.ndofs)
    A = rc.assembled("poisson", mesh, p, kappa, cvec)
    info = solve_and_check(op, h, A, b, u0, u0)
    print(f"{which} p={p} {kind}: {info['iterations']} iterations")


@pytest.mark.parametrize("p", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", KINDS)
def test_solve_mixed_boundary(p, kind):
    """Dirichlet on two sides with inhomogeneous values, prescribed normal flux through neumann_load on the other two"""
    from dolfinx_eqlb_amd.eqlb.bcs import fluxbc
    dm, mesh = setup("base")
    kappa = pc.kappa_of(mesh.ncells)
    sides = gk.side_facets(mesh)
    op, h, cvec = pair(dm, mesh, p, kappa, np.concatenate([sides[0], sides[1]]), kind)
    rng = np.random.default_rng(p)
    d = min(p, 3)
    f = rng.standard_normal(mesh.ncells * (d + 1) * (d + 2) // 2)
    be = primal.neumann_load(mesh, p, [fluxbc(lambda x, y: 1.0 + x + y * y, sides[2], scalar=True),
                                       fluxbc(lambda x, y: (np.sin(x), 2.0 + 0.0 * y), sides[3])])
    b = h.load(d, f, be)
    assert np.array_equal(bits(b), bits(op.load(d, f, be)))
    u0 = np.where(op.fixed, rng.standard_normal(op.ndofs), 0.0)
    start = np.where(op.fixed, u0, rng.standard_normal(op.ndofs))      # any start on the free rows
    A = rc.assembled("poisson", mesh, p, kappa, cvec)
    solve_and_check(op, h, A, b, u0, start)


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_solve_elasticity(p):
    """one case per p: cell-wise pi_1 and c, Dirichlet all around in both rows, against the galerkin-style assembly with
    the block-diagonal mass"""
    dm, mesh = setup("base")
    op, pi1, args = pm.statement("elasticity", mesh, p, "all")
    h = make_handle("elasticity", dm, p, pi1, args)
    cc = rc.c_of(mesh.ncells)
    op.set_reaction(cell_c=cc)
    h.set_reaction(cell_c=cc)
    b, u0, start = pm.solve_data(op, "elasticity", "reaction-base9", p, True)
    A = rc.assembled("elasticity", mesh, p, pi1, cc)
    u, info = h.solve(b, start, rtol=RTOL, maxit=20000)
    check_elasticity(op, A, b, u0, u, info, RTOL)
    u2, info2 = h.solve(b, start, rtol=RTOL, maxit=20000)
    assert np.array_equal(bits(u), bits(u2)) and info == info2


# ---- 5. the hierarchy ------------------------------------------------------------------------------------------------------
def levels(problem, name, p, cs):
    """(statements, handles, refinements) on levels_of(name), Dirichlet all around, reaction cs[l] (or None) on level l"""
    dms, refs = device_levels(name)
    meshes = [d.mesh for d in dms]
    links = [(r.parent_cell, r.node_parent_facet) for r in refs]
    coeff = pm.mc.coefficients(meshes, links, pc.kappa_of if problem == "poisson" else pm.ec.pi1_of)
    ops, hs = [], []
    for dm, m, k, c in zip(dms, meshes, coeff, cs):
        op, _, args = pm.statement(problem, m, p, "all", k)
        h = make_handle(problem, dm, p, k, args)
        if c is not None:
            op.set_reaction(cell_c=c)
            h.set_reaction(cell_c=c)
        ops.append(op)
        hs.append(h)
    return ops, hs, refs, meshes, coeff


FORMS = [dict(), dict(local=True), dict(coarse=True), dict(local=True, coarse=True)]


@pytest.mark.parametrize("name", ["disk70", "hole"])
@pytest.mark.parametrize("problem,p", [("poisson", 1), ("poisson", 2), ("elasticity", 1)])
def test_hierarchy_with_a_reaction_on_every_level(problem, name, p):
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.lsolver.multilevel import Hierarchy
    dms, _ = device_levels(name)
    cs = [rc.c_of(d.mesh.ncells, seed=31 + l) for l, d in enumerate(dms)]
    ops, hs, refs, meshes, coeff = levels(problem, name, p, cs)
    op = ops[-1]
    r = np.random.default_rng(pm.seed_of("reaction-hierarchy", problem, name, p)).standard_normal(op.fixed.size)
    plain_ops = levels(problem, name, p, [None] * len(dms))[0]
    z_plain = Hierarchy(plain_ops, refs).precondition(r)
    for form in FORMS:
        H = Hierarchy(ops, refs, **form)
        ml = cpp.Multilevel(hs, refs, **form)
        for call in range(2):
            z = ml.precondition(r)
            assert np.array_equal(bits(z), bits(H.precondition(r))), form
        if not form:
            assert not np.array_equal(z, z_plain)      # the reaction is in the diagonals
        if form.get("coarse"):
            ml.set_coarse(True)                        # a renewed factor is the statement's
            same_factor(ml, H)
            assert np.array_equal(bits(ml.precondition(r)), bits(z))
        ml.close()
    # the solve converges, with the true-residual confirmation, for stiffness + mass
    ml = cpp.Multilevel(hs, refs, local=True, coarse=True)
    b, u0, start = pm.solve_data(op, problem, "reaction-" + name, p)
    u, info = ml.solve(b, start, rtol=RTOL, maxit=2000)
    assert info["converged"] == 1 and info["breakdown"] == 0
    n = op.fixed.size
    rs = op.residual(b, u)                             # the statement's residual, with the term
    rn, tol = np.sqrt(np.sum(rs * rs)), RTOL * op.reference_norm(b, u0)
    assert rn <= tol * (1.0 + n * rc.U) and abs(info["rnorm"] - rn) <= n * rc.U * rn
    assert np.array_equal(bits(u[op.fixed]), bits(u0[op.fixed]))
    A = rc.assembled(problem, meshes[-1], p, coeff[-1], cs[-1])
    free = np.nonzero(~op.fixed)[0]
    ra = (b - A @ u)[free]                             # ... and that of the assembled stiffness + mass
    assert np.sqrt(ra @ ra) <= tol * (1.0 + 1e-3)
    _, jac = hs[-1].solve(b, start, rtol=RTOL, maxit=20000)
    print(f"{problem} {name} p={p}: hierarchy {info['iterations']} iterations, Jacobi {jac['iterations']}")
    ml.close()


@pytest.mark.parametrize("problem,p", [("poisson", 2), ("elasticity", 1)])
def test_reaction_set_after_the_hierarchy_was_created(problem, p):
    """the next precondition sees the new diagonals; the dense factor of level 0 is a snapshot until set_coarse(True)"""
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.lsolver.multilevel import Hierarchy
    name = "hole"
    dms, _ = device_levels(name)
    ops, hs, refs, _, _ = levels(problem, name, p, [None] * len(dms))
    r = np.random.default_rng(pm.seed_of("reaction-late", problem, p)).standard_normal(ops[-1].fixed.size)
    ml = cpp.Multilevel(hs, refs)
    mlc = cpp.Multilevel(hs, refs, coarse=True)
    z0, zc0 = ml.precondition(r), mlc.precondition(r)
    assert np.array_equal(bits(z0), bits(Hierarchy(ops, refs).precondition(r)))
    for l, (op, h) in enumerate(zip(ops, hs)):
        c = rc.c_of(op.mesh.ncells, seed=7 + l)
        op.set_reaction(cell_c=c)
        h.set_reaction(cell_c=c)
    z1 = ml.precondition(r)
    assert not np.array_equal(z1, z0)
    assert np.array_equal(bits(z1), bits(Hierarchy(ops, refs).precondition(r)))
    # the factor still belongs to the operator without the term: the statement with the old factor on level 0
    H = Hierarchy(ops, refs, coarse=True)
    plain0 = levels(problem, name, p, [None] * len(dms))[0]
    H._factor = Hierarchy(plain0, refs, coarse=True).coarse_factor()
    assert np.array_equal(bits(mlc.precondition(r)), bits(H.precondition(r)))
    mlc.set_coarse(True)
    Hn = Hierarchy(ops, refs, coarse=True)
    same_factor(mlc, Hn)
    zc1 = mlc.precondition(r)
    assert np.array_equal(bits(zc1), bits(Hn.precondition(r))) and not np.array_equal(zc1, zc0)
    ml.close()
    mlc.close()
