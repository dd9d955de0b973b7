"""The Poisson chain with a diffusion tensor on the device: u = sin(pi x) sin(pi y) on the unit square with the constant
rotated tensor D = R(pi / 6) diag(1, eps) R^T, eps in {1, 1e-2, 1e-4}, and the analytic f (tests/diffusion_cases.py).
Three levels: PrimalPoisson + set_diffusion solved to rtol 1e-12 -> primal_flux_dg(cell_D=) -> project_dg (f) -> SE
equilibration at k = 2, 3 -> estimate(cell_D=) -> oscillation with the weight 1 / sqrt(lambda_min(D)) ->
indicator_total(pair_last_two=True) -> mark_doerfler -> refine -> prolong of u_h, prolong_dg of D at degree 0 with
bs = 3 IN DEVICE MEMORY (the handle of the next level takes the pointer: set_diffusion_raw) -> the next solve from the
prolonged start through Multilevel(local=True, coarse=True).

On every level eta^2 = sum (sqrt sig2 + oscillation)^2 >= || D^(1/2) grad(u - u_h) ||^2, the error by a quadrature of
degree 2 p + 6 on the host; the effectivity is printed and not bounded from above.  The two device totals equal those of
the host chain on the same mesh (diffusion_cases.host_level: sparse direct solve of the matrix assembled by quadrature,
the oracle, the numpy statements) within 1e-9 relative, the figure of tests/test_gpu_shear_chain.py.  The solves stop at
rtol 1e-12: at k = 3 a relative residual of 1e-13 lies below what the recurrence reaches (the statement's pcg stalls
between 1e-12 and 6e-11 there, whatever the preconditioner), and with the statement's pcg at 1e-12 in the place of the
direct solve the totals of the host chain move by at most 1.3e-10 (k = 3, eps = 1e-4, level 2).
Measured on an MI355X: the device totals deviate from the host chain's by at most 4.1e-11 (sig2) and 1.4e-12 (oscillation);
eta / e is 1.27 ... 1.46 at eps = 1, 7.9 ... 9.1 at 1e-2 and 78 ... 91 at 1e-4; the solves take 6 ... 394 iterations, each in
one call.

With cell_D left out of estimate at eps = 1e-2, the total of the unweighted cell_sig2 falls below the squared error on at
least one level.  The host statement shows it first (tests/test_primal_diffusion_host.py:
test_host_chain_gives_a_guaranteed_bound_and_the_unweighted_norm_does_not: levels 1 and 2, 0.91 ... 0.97 of the error), so
eps did not have to be lowered."""

import numpy as np
import pytest

import diffusion_cases as dc
from dolfinx_eqlb_amd.lsolver import primal

pytestmark = pytest.mark.gpu

U = dc.U
RTOL = 1e-12


def solve_restarted(solve, b, u, maxit=2000, calls=3):
    """a solve to RTOL, started again from its own iterate while it has not converged (see
    tests/test_gpu_shear_chain.py: after a residual replacement the kept directions may stall just above the tolerance)"""
    for call in range(calls):
        u, info = solve(b, u, rtol=RTOL, maxit=maxit)
        if info["converged"] == 1:
            break
    return u, info, call + 1


@pytest.mark.parametrize("eps", dc.EPS)
@pytest.mark.parametrize("k", [2, 3])
def test_three_levels_give_a_guaranteed_bound(oracle_mod, k, eps):
    import torch
    from dolfinx_eqlb_amd import cpp
    from synthetic import facet_types
    dev = torch.device("cuda:0")
    ex = dc.exact(eps)
    dm = cpp.DeviceMesh(dc.chain_mesh())
    d_D = torch.from_numpy(dc.tensor_of("fixed", dm.mesh, eps)).to(dev)          # [ncells, 3] in device memory
    solvers, refs, keep = [], [], []
    u0, below = None, []
    for level in range(3):
        mesh = dm.mesh
        D = d_D.cpu().numpy().reshape(-1, 3)
        assert np.array_equal(D, dc.tensor_of("fixed", mesh, eps))              # the children took the tensor of the cell
        h = cpp.PrimalPoisson(dm, k)
        bf = mesh.boundary_facets().astype(np.int32)
        h.set_dirichlet(bf)
        torch.cuda.synchronize()
        h.set_diffusion_raw(d_D.data_ptr())
        solvers.append(h)
        keep.append((dm, d_D))
        host = dc.host_level(oracle_mod, mesh, k, eps, D)
        qp, qw = host["qp"], host["qw"]
        fv = ex["f"](*dc.points(mesh, qp))
        fh = cpp.project_dg(dm, k - 1, qp, qw, fv[None, :, :, None])
        b = h.load(k - 1, fh[0])
        if level == 0:
            u, info, calls = solve_restarted(h.solve, b, np.zeros(h.ndofs))
        else:
            ml = cpp.Multilevel(solvers, refs, local=True, coarse=True)
            op = primal.PoissonOperator(mesh, k)
            op.set_dirichlet(bf)
            u, info, calls = solve_restarted(ml.solve, b, np.where(op.fixed, 0.0, u0))
            ml.close()
        assert info["converged"] == 1 and info["breakdown"] == 0, info
        cd = dm.lagrange_dofmap(k)[0]
        assert np.array_equal(cd, host["cd"])
        G = cpp.primal_flux_dg(dm, k, k - 1, cd, u, cell_D=D)
        eq = cpp.SemiExplicitEquilibrator(dm, k, 1)
        eq.set_boundary(facet_types(mesh, None))
        x = eq.equilibrate_host(G, fh)
        div2, sig2, _ = cpp.estimate(dm, k, x, G, fh, cell_D=D)
        _, plain, _ = cpp.estimate(dm, k, x, G, fh)
        osc = cpp.oscillation(dm, k, x, G, qp, qw, fv[None], primal.diffusion_oscillation_weight(D))
        eta2, totals = cpp.indicator_total([sig2[0], osc[0]], pair_last_two=True)
        err2 = dc.energy_error2(mesh, k, u, cd.astype(np.int64), eps, D)
        rel = np.sqrt(div2.sum()) / np.sqrt(np.sum(fh ** 2))
        ref = (host["sig2"].sum(), host["osc"].sum())
        print(f"k={k} eps={eps} level {level}: {mesh.ncells} cells, {info['iterations']} iterations in the last of {calls} "
              f"calls, eta / e = {np.sqrt(totals[2] / err2):.4f}, unweighted sqrt(sum sig2) / e = "
              f"{np.sqrt(plain.sum() / err2):.4f}, relative div residual {rel:.2e}; totals device {totals[:2]}, host {ref}, "
              f"relative deviation {[abs(t - r) / r for t, r in zip(totals[:2], ref)]}")
        assert totals[2] >= err2
        assert rel < 1e-9
        assert abs(err2 - host["err2"]) <= 1e-9 * err2
        for name, got, want in zip(("sig2", "osc"), totals[:2], ref):
            assert abs(got - want) <= 1e-9 * want, (name, got, want)
        below.append(plain.sum() < err2)
        if level == 2:
            break
        marked, _ = cpp.mark_doerfler(eta2, dc.CHAIN_THETA)
        ref_ = dm.refine(marked, keep_plan=True)
        u0 = np.ascontiguousarray(ref_.prolong(k, u)).ravel()
        d_D = ref_.prolong_dg(0, d_D.reshape(-1), bs=3)                          # device in, device out
        assert d_D.is_cuda and d_D.numel() == 3 * ref_.dmesh.mesh.ncells
        refs.append(ref_)
        dm = ref_.dmesh
    if eps == 1e-2:
        assert any(below)
