"""The adaptive chain with a reaction term, on the device, in the shape of test_adaptive_loop_on_the_device
(tests/test_gpu_primal_solve.py) with two levels: -div(grad u) + c u = f with a cell-wise c in [0, 1000] is solved from
the prolonged start, the flux G = primal_flux_dg(u) is equilibrated against
    rhs = Pi_d f - primal_value_dg(u, c)
and the equilibration conditions are checked with that test's own figures: the divergence residual relative to the
right-hand side < 1e-9 and the largest facet jump < 1e-9.

The two figures cannot pass vacuously: with the reaction part left out of rhs the data are not compatible with G on the
interior patches, and the defect has to show.  WHERE it shows depends on the equilibrator.  The reference algorithm
(the CPU oracle, se_reconstruct) walks round a patch and does not close the loop: its flux has a facet jump, which must
exceed 1e-6 here (jump_residual of the oracle's flux of the SAME G and Pi_d f).  The device kernel gives both cells of
a facet the one set of facet moments, so its flux has no jump by construction (measured: 3e-16) and the defect lands in
the divergence of a cell of the patch: there the relative divergence residual must exceed 1e-6.  Both are asserted.
c is carried to the refined mesh by prolong_dg as every cell-wise coefficient is.

Then one implicit heat step, twice: (u_new - u_old) / tau - div(grad u_new) = f, the load f + u_old / tau through a
PrimalValue of u_old.  tau = 0.5 is ten times the diffusion time 1 / (2 pi^2) of the unit square, so the first step
takes the state most of the way to the steady state and the second step starts close to its solution: from there it
must need fewer iterations than from zero (the statement's pcg on a like mesh: 68 against 75; the relative tolerance
refers to the same reference norm for both starts).

(k, p) = (2, 2) and (3, 2), the data in DG_{k-1}: at k = 1 the check does not hold (the hat function is not in P_0)."""

import numpy as np
import pytest

from dolfinx_eqlb_amd.lsolver import PrimalValue, local_projection, primal
from dolfinx_eqlb_amd.mesh import create_unit_square
from test_gpu_primal_solve import bits

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
_KEEP = []


@pytest.mark.parametrize("k,p", [(2, 2), (3, 2)])
def test_chain_with_a_reaction_term_and_two_heat_steps(oracle_mod, k, p):
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
    from dolfinx_eqlb_amd.eqlb import check_eqlb_conditions as chk
    from synthetic import facet_types
    import test_estimator_bound as teb
    d = k - 1
    qp, qw = make_quadrature_triangle(2 * k + 6)
    dm = cpp.DeviceMesh(create_unit_square(4, shuffle_seed=3, perturb=0.15))
    c = np.random.default_rng(10 * k + p).uniform(0.0, 1000.0, dm.mesh.ncells)
    c[::6] = 0.0
    u = eq_old = ref = None
    for level in range(2):
        mesh = dm.mesh
        J, _, _ = chk.cell_geometry(mesh)
        x0 = mesh.x[mesh.cell_nodes[:, 0], :2]
        xq = x0[:, None, :] + np.einsum("cij,qj->cqi", J, qp)
        fh = cpp.project_dg(dm, d, qp, qw, teb.f_ex(xq[..., 0], xq[..., 1])[None, :, :, None])[0]
        pp = cpp.PrimalPoisson(dm, p)
        pp.set_dirichlet(mesh.boundary_facets())
        pp.set_reaction(cell_c=c)
        b = pp.load(d, fh)
        u, info = pp.solve(b, np.zeros(pp.ndofs) if u is None else u, rtol=1e-12, maxit=5000)
        assert info["converged"] == 1
        cd, ndofs = dm.lagrange_dofmap(p)
        G = cpp.primal_flux_dg(dm, p, d, cd, u)[0]
        cu = cpp.primal_value_dg(dm, p, d, cd, u, coeff=c)[0]
        assert np.array_equal(bits(cu), bits(primal.value_dg(p, d, cd, u, c)[0]))
        rhs = fh - cu
        eq = cpp.SemiExplicitEquilibrator(dm, k, 1)
        if level == 0:
            eq.set_boundary(facet_types(mesh, None))
        else:
            eq.carry_boundary(eq_old, ref)
        x = eq.equilibrate_host(G[None], rhs[None])
        div2, sig2, jump = cpp.estimate(dm, k, x, G[None], rhs[None])
        rel = np.sqrt(div2.sum()) / np.sqrt(np.sum(rhs ** 2))
        # the reaction part left out: the defect shows - in the jump of the reference algorithm, in the divergence on
        # the device (the head of this file)
        x_f = eq.equilibrate_host(G[None], fh[None])
        div2_f, _, jump_f = cpp.estimate(dm, k, x_f, G[None], fh[None])
        rel_f = np.sqrt(div2_f.sum()) / np.sqrt(np.sum(fh ** 2))
        ft = facet_types(mesh, None)
        x_o = oracle_mod.se_reconstruct(mesh, k, ft, G[None], fh[None])[0]
        jump_o = np.abs(chk.jump_residual(mesh, k, x_o, G)).max()
        jump_ok = np.abs(chk.jump_residual(mesh, k, oracle_mod.se_reconstruct(mesh, k, ft, G[None], rhs[None])[0], G)).max()
        print(f"k={k} p={p} level {level}: {mesh.ncells} cells, {info['iterations']} iterations, relative div residual "
              f"{rel:.2e}, jump {jump.max():.2e} (oracle on the same data: jump {jump_ok:.2e}); without the reaction "
              f"part: device relative div residual {rel_f:.2e}, jump {jump_f.max():.2e}; oracle jump {jump_o:.2e}")
        assert rel < 1e-9 and jump.max() < 1e-9 and jump_ok < 1e-9
        assert jump_o > 1e-6
        assert rel_f > 1e-6
        if level == 1:
            break
        marked, _ = cpp.mark_doerfler(sig2[0], 0.5)
        ref = dm.refine(marked, keep_plan=True)
        u = ref.prolong(p, u)
        c = np.ascontiguousarray(ref.prolong_dg(0, c)).ravel()
        assert u.size == ref.dmesh.lagrange_dofmap(p)[1] and c.size == ref.dmesh.mesh.ncells
        eq_old, dm_old, dm = eq, dm, ref.dmesh
        _KEEP.append((dm_old, eq_old, ref))   # the plan reads the old handles: they outlive the level

    # one implicit heat step, twice, on the refined mesh: u_old is the solution above
    tau = 0.5
    hh = cpp.PrimalPoisson(dm, p)
    hh.set_dirichlet(mesh.boundary_facets())
    hh.set_reaction(1.0 / tau)
    op = primal.PoissonOperator(mesh, p)
    op.set_dirichlet(mesh.boundary_facets())
    op.set_reaction(1.0 / tau)
    inv_tau = np.full(mesh.ncells, 1.0 / tau)
    zero = np.zeros(hh.ndofs)

    def step(u_old, start):
        mass = local_projection(dm, d, [PrimalValue(p, cd, u_old, inv_tau)], bs=1)[0]
        assert np.array_equal(bits(mass), bits(primal.value_dg(p, d, cd, u_old, inv_tau)[0]))
        b = hh.load(d, fh + mass)
        assert np.array_equal(bits(b), bits(op.load(d, fh + mass)))
        un, inf = hh.solve(b, start, rtol=1e-10, maxit=5000)
        assert inf["converged"] == 1 and inf["breakdown"] == 0
        r = op.residual(b, un)                              # the statement's residual, with the term u / tau
        assert np.sqrt(np.sum(r * r)) <= 1e-10 * op.reference_norm(b, zero) * (1.0 + op.ndofs * U)
        return un, inf["iterations"]

    u1, it1 = step(u, zero)
    assert np.abs(u1 - u).max() > 1e-6 * np.abs(u).max()     # (the state moves: u is no steady state of the heat equation)
    u2, it2 = step(u1, u1)
    _, it2_cold = step(u1, zero)
    print(f"k={k} p={p}: heat steps at tau = {tau}: {it1} iterations from zero, second step {it2} from the first, "
          f"{it2_cold} from zero")
    assert it2 < it2_cold
