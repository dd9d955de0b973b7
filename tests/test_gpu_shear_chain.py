"""The elasticity chain with a cell-wise shear modulus on the bimaterial square of tests/shear_cases.py, on the device:
PrimalElasticity + set_shear solved to rtol 1e-13 -> primal_stress_dg(cell_pi1, cell_mu) -> project_dg -> stress
equilibration with Korn constants -> estimate_stress(cell_pi1, cell_mu) -> oscillation with korn / sqrt(mu) ->
indicator_total(pair_last_two=True).  The bound eta >= e holds against the exact solution, and each of the three totals
agrees with the host chain (sparse direct solve of the matrix with mu inside the integral, oracle with weak symmetry
and Korn constants, numpy statements) within 1e-9 relative, the margin of test_gpu_elasticity_pipeline_bound.  The host
chain satisfies the bound for every (mu2, k, n) of tests/test_primal_shear_host.py
(test_bimaterial_guaranteed_upper_bound), so it is asserted here for all four cases.

Then two Doerfler steps on the device: mark, refine, prolong(bs=2), prolong_dg of mu and pi_1 (a DG_0 coefficient
crosses a refinement as every cell-wise coefficient does; the children of a cell lie on its side of the interface), a new
handle with set_shear, and the solve from the prolonged start through Multilevel(local=True, coarse=True).  The solve
converges with its true residual confirmed by the statement, and the divergence residual of the equilibrated rows stays
below 1e-9 relative on every level."""

import numpy as np
import pytest

import shear_cases as sc
from dolfinx_eqlb_amd.lsolver import primal

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
RTOL = 1e-13


def level_data(cpp, dm, k, mu2, cell_pi1, cell_mu, qp, qw):
    """the projected right-hand side and the point values of f on the mesh of dm, the side of a cell taken from mu"""
    mesh = dm.mesh
    right = cell_mu > 1.0 if mu2 != 1 else cell_pi1 > sc.PI_LEFT
    ex = sc.exact(mu2)
    xq, yq = sc.points(mesh, qp)
    fv = np.stack([sc.side_fn(mesh, right, ex["f"][r])(xq, yq) for r in range(2)])
    fh = cpp.project_dg(dm, k - 1, qp, qw, fv[:, :, :, None])
    return fv, fh


def solve_restarted(h, b, u, maxit=1000, calls=6):
    """h.solve to rtol 1e-13, started again from its own iterate while it has not converged.  At k = 3, mu2 = 1000 the
    Jacobi-preconditioned CG does not get below 2e-12 of the reference norm in one call, however long it runs (20 000
    iterations on the device; the statement's pcg the same: 6.1e-13 after 1000): once the recurrence residual has been
    replaced by the true one, the search directions kept from before no longer fit it.  A call started from the
    iterate builds them anew and converges in a few iterations (the statement: 4).  The other three cases converge in
    the first call (212 iterations at k = 2, mu2 = 10)."""
    for call in range(calls):
        u, info = h.solve(b, u, rtol=RTOL, maxit=maxit)
        if info["converged"] == 1:
            break
    return u, info, call + 1


def equilibrate(cpp, dm, k, ft, G, fh):
    eq = cpp.SemiExplicitEquilibrator(dm, k, 2, reconstruct_stress=True, estimate_korn=True)
    eq.set_boundary(ft)
    x, ck2 = eq.equilibrate_host_with_kornconst(G, fh)
    div2, _, _ = cpp.estimate(dm, k, x, G, fh)
    rel = np.sqrt(div2.sum()) / np.sqrt(np.sum(fh ** 2))
    return x, np.sqrt(ck2), rel


@pytest.mark.parametrize("mu2", [10, 1000])
@pytest.mark.parametrize("k", [2, 3])
def test_bimaterial_chain_bound_and_two_adaptive_steps(oracle_mod, k, mu2):
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
    from synthetic import facet_types
    n = 8
    P = sc.problem(n, k, mu2)
    mesh = P["mesh"]
    host = sc.host_terms(oracle_mod, P, k)
    assert sc.estimate(*host[:3]) / P["err"] >= 1.0 - 1e-10          # the host chain satisfies the bound here
    qp, qw = make_quadrature_triangle(2 * k + 6)
    dm = cpp.DeviceMesh(mesh)
    cell_pi1, cell_mu = P["cell_pi1"], P["cell_mu"]
    solver = cpp.PrimalElasticity(dm, k, cell_pi1=cell_pi1)
    solver.set_shear(cell_mu=cell_mu)
    cd = dm.lagrange_dofmap(k)[0]
    assert np.array_equal(cd, P["cd"])                               # the numbering the host load b is written in
    bf = mesh.boundary_facets().astype(np.int32)
    solver.set_dirichlet(bf, bf)
    u, info, calls = solve_restarted(solver, P["b"], np.zeros(2 * solver.ndofs))
    assert info["converged"] == 1, info
    G = cpp.primal_stress_dg(dm, k, k - 1, cd, u, cell_pi1=cell_pi1, cell_mu=cell_mu)
    fv, fh = level_data(cpp, dm, k, mu2, cell_pi1, cell_mu, qp, qw)
    x, korn, rel = equilibrate(cpp, dm, k, P["ft"], G, fh)
    energy, wsym, asym = cpp.estimate_stress(dm, k, x, korn, cell_pi1=cell_pi1, cell_mu=cell_mu)
    osc = cpp.oscillation(dm, k, x, G, qp, qw, fv, korn / np.sqrt(cell_mu)).sum(axis=0)
    eta2, totals = cpp.indicator_total([energy, wsym, osc], pair_last_two=True)
    eta = float(np.sqrt(totals[3]))
    print(f"k={k} mu2={mu2}: {info['iterations']} iterations in the last of {calls} calls, eta_device / e = {eta / P['err']:.4f}, relative div residual "
          f"{rel:.2e}; totals device {totals[:3]}, host {[float(t.sum()) for t in host[:3]]}")
    assert eta / P["err"] >= 1.0 - 1e-10
    assert rel < 1e-9
    for name, dev, ref in zip(("energy", "wsym", "osc"), totals[:3], host[:3]):
        assert abs(dev - ref.sum()) <= 1e-9 * ref.sum(), (name, dev, ref.sum())

    # ---- two Doerfler steps on the device ----
    solvers, refs, keep = [solver], [], [dm]
    for step in range(2):
        marked, _ = cpp.mark_doerfler(eta2, 0.5)
        ref = dm.refine(marked, keep_plan=True)
        u0 = np.ascontiguousarray(ref.prolong(k, u, bs=2)).ravel()
        cell_mu = np.ascontiguousarray(ref.prolong_dg(0, cell_mu)).ravel()
        cell_pi1 = np.ascontiguousarray(ref.prolong_dg(0, cell_pi1)).ravel()
        dm = ref.dmesh
        mesh = dm.mesh
        assert np.array_equal(cell_mu, P["cell_mu"][_root(refs + [ref])])     # the children take the value of the cell
        xc = mesh.x[mesh.cell_nodes, 0]
        assert np.all(xc[cell_mu > 1.0] >= 0.5) and np.all(xc[cell_mu == 1.0] <= 0.5)     # no cell straddles
        h = cpp.PrimalElasticity(dm, k, cell_pi1=cell_pi1)
        h.set_shear(cell_mu=cell_mu)
        bf = mesh.boundary_facets().astype(np.int32)
        h.set_dirichlet(bf, bf)
        solvers.append(h)
        refs.append(ref)
        keep.append(dm)
        fv, fh = level_data(cpp, dm, k, mu2, cell_pi1, cell_mu, qp, qw)
        b = h.load(k - 1, fh)
        op = primal.ElasticityOperator(mesh, k, cell_pi1=cell_pi1)
        op.set_shear(cell_mu=cell_mu)
        op.set_dirichlet(bf, bf)
        start = np.where(op.fixed, 0.0, u0)
        ml = cpp.Multilevel(solvers, refs, local=True, coarse=True)
        u, info = ml.solve(b, start, rtol=1e-12, maxit=5000)
        ml.close()
        assert info["converged"] == 1 and info["breakdown"] == 0, info
        nrow = op.fixed.size
        rs = op.residual(b, u)                                       # the statement's residual, with the modulus
        rn, tol = np.sqrt(np.sum(rs * rs)), 1e-12 * op.reference_norm(b, np.zeros(nrow))
        assert rn <= tol * (1.0 + nrow * U) and abs(info["rnorm"] - rn) <= nrow * U * rn
        cd = dm.lagrange_dofmap(k)[0]
        G = cpp.primal_stress_dg(dm, k, k - 1, cd, u, cell_pi1=cell_pi1, cell_mu=cell_mu)
        ft = np.repeat(facet_types(mesh, None), 2, axis=0)
        x, korn, rel = equilibrate(cpp, dm, k, ft, G, fh)
        energy, wsym, _ = cpp.estimate_stress(dm, k, x, korn, cell_pi1=cell_pi1, cell_mu=cell_mu)
        osc = cpp.oscillation(dm, k, x, G, qp, qw, fv, korn / np.sqrt(cell_mu)).sum(axis=0)
        eta2, totals = cpp.indicator_total([energy, wsym, osc], pair_last_two=True)
        err = sc.energy_error(mesh, k, u.reshape(-1, 2), cd.astype(np.int64), sc.exact(mu2), cell_pi1, cell_mu,
                              cell_mu > 1.0)
        print(f"k={k} mu2={mu2} step {step + 1}: {mesh.ncells} cells, {info['iterations']} hierarchy iterations, relative "
              f"div residual {rel:.2e}, eta / e = {np.sqrt(totals[3]) / err:.4f}")
        assert rel < 1e-9


def _root(refs):
    """the cell of the base mesh every cell of the last level descends from"""
    root = None
    for r in refs:
        pc = np.asarray(r.parent_cell)
        root = pc if root is None else root[pc]
    return root
