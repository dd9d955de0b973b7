"""The Poisson chain with a Robin side on the device, in the shape of tests/test_gpu_diffusion_chain.py: the model problem
of tests/robin_cases.py (u = sin(omega x) sin(pi y), tan(omega) = -omega / alpha, alpha = 1: -du/dn = alpha u on x = 1,
u = 0 on the other sides).  Three Doerfler levels at k = 2, 3: PrimalPoisson + set_robin (carried by
Refinement.carry_robin) solved to rtol 1e-12 -> primal_flux_dg -> project_dg (f) -> robin_flux (the flux condition
alpha u_h at the points of a Gauss rule) -> update_flux_bc on the facets of type EQLB_FACET_ESSNT_DUAL -> SE
equilibration -> estimate -> oscillation -> indicator_total(pair_last_two=True) -> mark_doerfler -> refine -> prolong
of u_h -> the next solve from the prolonged start through Multilevel(local=True, coarse=True).

On every level eta^2 >= |||u - u_h|||^2 = || grad e ||^2 + || alpha^(1/2) e ||^2 on the Robin side (quadrature of degree
2 k + 6 on the host), and the two device totals equal those of the host chain on the same mesh (robin_cases.host_level:
sparse direct solve of the matrix assembled by quadrature with the boundary mass, the oracle with boundary_values = the
moments of alpha u_h) within 1e-9 relative, the figure of tests/test_gpu_diffusion_chain.py.  At flux degree k = primal
degree the moments drop the top moment of alpha u_h: the omitted boundary oscillation is of higher order and not part
of the guarantee (tests/test_primal_robin_host.py)."""

import numpy as np
import pytest

import robin_cases as rb
from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
from dolfinx_eqlb_amd.eqlb.check_eqlb_conditions import cell_geometry

pytestmark = pytest.mark.gpu

RTOL = 1e-12
THETA = 0.5


def solve_restarted(solve, b, u, maxit=2000, calls=3):
    """a solve to RTOL, started again from its own iterate while it has not converged (tests/test_gpu_shear_chain.py)"""
    for call in range(calls):
        u, info = solve(b, u, rtol=RTOL, maxit=maxit)
        if info["converged"] == 1:
            break
    return u, info, call + 1


@pytest.mark.parametrize("k", [2, 3])
def test_three_levels_give_a_guaranteed_bound(oracle_mod, k):
    import galerkin as gk
    from dolfinx_eqlb_amd import cpp
    dm = cpp.DeviceMesh(rb.chain_mesh(8))
    solvers, refs = [], []
    u0 = None
    qp, qw = make_quadrature_triangle(2 * k + 6)
    s, wq = rb.flux_rule(k)
    for level in range(3):
        mesh = dm.mesh
        left, bottom, right, top = rb.sides(mesh)
        dirichlet = np.concatenate([left, bottom, top])
        h = cpp.PrimalPoisson(dm, k)
        h.set_dirichlet(dirichlet)
        if level == 0:
            h.set_robin(right, alpha=rb.ALPHA)
        else:
            refs[-1].carry_robin(solvers[-1], h)
        robin = h.robin_list()[0]
        assert np.array_equal(np.sort(robin), right) and np.all(h.robin_list()[1] == rb.ALPHA)
        solvers.append(h)
        host = rb.host_level(oracle_mod, mesh, k)
        J = cell_geometry(mesh)[0]
        xq = mesh.x[mesh.cell_nodes[:, 0], :2][:, None, :] + np.einsum("cij,qj->cqi", J, qp)
        fv = rb.f_ex(xq[..., 0], xq[..., 1])
        fh = cpp.project_dg(dm, k - 1, qp, qw, fv[None, :, :, None])
        b = h.load(k - 1, fh[0])
        if level == 0:
            u, info, calls = solve_restarted(h.solve, b, np.zeros(h.ndofs))
        else:
            ml = cpp.Multilevel(solvers, refs, local=True, coarse=True)
            u, info, calls = solve_restarted(ml.solve, b, u0)
            ml.close()
        assert info["converged"] == 1 and info["breakdown"] == 0, info
        cd = dm.lagrange_dofmap(k)[0]
        G = cpp.primal_flux_dg(dm, k, k - 1, cd, u)
        ft = np.zeros((1, mesh.nfacets), dtype=np.int8)
        ft[0, mesh.boundary_facets()] = 1
        ft[0, robin] = 2
        eq = cpp.SemiExplicitEquilibrator(dm, k, 1)
        eq.set_boundary(ft)
        eq.update_flux_bc(0, robin, h.robin_flux(u, s), s, wq, vector=False)
        x = eq.equilibrate_host(G, fh)
        div2, sig2, _ = cpp.estimate(dm, k, x, G, fh)
        osc = cpp.oscillation(dm, k, x, G, qp, qw, fv[None])
        eta2, totals = cpp.indicator_total([sig2[0], osc[0]], pair_last_two=True)
        err2 = gk.energy_error(mesh, k, u, cd.astype(np.int64), rb.grad_ex) ** 2 \
            + rb.boundary_error2(mesh, k, right, rb.ALPHA, u)
        rel = np.sqrt(div2.sum()) / np.sqrt(np.sum(fh ** 2))
        ref = (host["sig2"].sum(), np.sum(host["osc"] ** 2))
        print(f"k={k} level {level}: {mesh.ncells} cells, {info['iterations']} iterations in the last of {calls} calls, "
              f"eta / e = {np.sqrt(totals[2] / err2):.4f}, relative div residual {rel:.2e}; totals device {totals[:2]}, "
              f"host {ref}, relative deviation {[abs(t - r) / r for t, r in zip(totals[:2], ref)]}")
        assert totals[2] >= err2
        assert rel < 1e-9
        assert abs(err2 - host["err2"]) <= 1e-9 * err2
        for name, got, want in zip(("sig2", "osc"), totals[:2], ref):
            assert abs(got - want) <= 1e-9 * want, (name, got, want)
        if level == 2:
            break
        marked, _ = cpp.mark_doerfler(eta2, THETA)
        refs.append(dm.refine(marked, keep_plan=True))
        u0 = np.ascontiguousarray(refs[-1].prolong(k, u)).ravel()
        dm = refs[-1].dmesh
