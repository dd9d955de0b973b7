"""The P_p Poisson solve on the device (cpp.PrimalPoisson, csrc/eqlb_primal_solve.hip) against its numpy statement
(dolfinx_eqlb_amd/lsolver/primal.py): operator, load, diagonal and residual bit for bit; the CG against the statement's
residual and a direct solve, with derived bounds; the limits of the iteration; a caller's stream; and the adaptive loop
of the reference's demos closed on the device.

The base mesh create_unit_square(9, shuffle_seed=3, perturb=0.15) has 324 cells - more than one workgroup of 256, the
smallest size at which the block hand-over of the cell kernel, the sum pass and the reduction is exercised - and is
also used refined once on the device at refine_cases.level_marks.  kappa is log-uniform in [1, 100] per cell."""

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import galerkin as gk
import primal_cases as pc
from dolfinx_eqlb_amd.lsolver import primal
from dolfinx_eqlb_amd.mesh import create_unit_square

pytestmark = pytest.mark.gpu

U = pc.U
_CACHE = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def setup(which):
    """(DeviceMesh, mesh) of the base mesh or of the base mesh refined once on the device"""
    if which not in _CACHE:
        from dolfinx_eqlb_amd import cpp
        from refine_cases import level_marks
        base = create_unit_square(9, shuffle_seed=3, perturb=0.15)
        assert base.ncells == 324
        dm = cpp.DeviceMesh(base)
        if which == "refined":
            ref = dm.refine(level_marks(base.ncells, 1))
            _CACHE["_keep"] = dm
            dm = ref.dmesh
        _CACHE[which] = (dm, dm.mesh)
    return _CACHE[which]


def problem(which, p):
    """the statement, the handle and the data of one (mesh, p), computed once"""
    key = (which, p)
    if key not in _CACHE:
        from dolfinx_eqlb_amd import cpp
        dm, mesh = setup(which)
        rng = np.random.default_rng(17 * p + len(which))
        kappa = pc.kappa_of(mesh.ncells)
        op = primal.PoissonOperator(mesh, p, kappa)
        op.set_dirichlet(mesh.boundary_facets())
        d = min(p, 3)
        f = rng.standard_normal(mesh.ncells * (d + 1) * (d + 2) // 2)
        e = rng.standard_normal(op.ndofs)
        u = rng.standard_normal(op.ndofs)
        h = cpp.PrimalPoisson(dm, p, kappa)
        h.set_dirichlet(mesh.boundary_facets())
        assert h.ndofs == op.ndofs
        _CACHE[key] = dict(dm=dm, mesh=mesh, kappa=kappa, op=op, h=h, d=d, f=f, e=e, u=u, b=op.load(d, f, e))
    return _CACHE[key]


# ---- 1. bit for bit --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["base", "refined"])
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_statements_bit_for_bit_host_memory(which, p):
    c = problem(which, p)
    op, h, u, b = c["op"], c["h"], c["u"], c["b"]
    for call in range(2):   # a second call gives the same bits
        assert np.array_equal(bits(h.apply(u)), bits(op.apply(u)))
        assert np.array_equal(bits(h.apply(u, masked=True)), bits(op.apply(u, masked=True)))
        assert np.array_equal(bits(h.load(c["d"], c["f"])), bits(op.load(c["d"], c["f"])))
        assert np.array_equal(bits(h.load(c["d"], c["f"], c["e"])), bits(b))
        assert np.array_equal(bits(h.diagonal()), bits(op.diagonal()))
        r, rn, nb = h.residual(b, u, norms=True)
        rs = op.residual(b, u)
        assert np.array_equal(bits(r), bits(rs))
        # the norms are sums in another order: ndofs roundings
        assert abs(rn - np.sqrt(np.sum(rs * rs))) <= op.ndofs * U * rn
        assert abs(nb - op.reference_norm(b, u)) <= op.ndofs * U * nb
        assert np.array_equal(bits(h.residual(b, u)), bits(rs))


@pytest.mark.parametrize("which", ["base", "refined"])
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_statements_bit_for_bit_device_memory(which, p):
    import torch
    c = problem(which, p)
    op, h, b = c["op"], c["h"], c["b"]
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    u, bb, f, e = t(c["u"]), t(b), t(c["f"]), t(c["e"])
    out = torch.full((op.ndofs,), float("nan"), dtype=torch.float64, device=dev)
    norms = torch.full((2,), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    for call in range(2):
        h.apply_raw(u.data_ptr(), out.data_ptr(), False)
        assert np.array_equal(bits(out.cpu().numpy()), bits(op.apply(c["u"])))
        h.apply_raw(u.data_ptr(), out.data_ptr(), True)
        assert np.array_equal(bits(out.cpu().numpy()), bits(op.apply(c["u"], masked=True)))
        h.load_raw(c["d"], f.data_ptr(), e.data_ptr(), out.data_ptr())
        assert np.array_equal(bits(out.cpu().numpy()), bits(b))
        h.load_raw(c["d"], f.data_ptr(), None, out.data_ptr())
        assert np.array_equal(bits(out.cpu().numpy()), bits(op.load(c["d"], c["f"])))
        h.diagonal_raw(out.data_ptr())
        assert np.array_equal(bits(out.cpu().numpy()), bits(op.diagonal()))
        h.residual_raw(bb.data_ptr(), u.data_ptr(), out.data_ptr(), norms.data_ptr())
        rs = op.residual(b, c["u"])
        assert np.array_equal(bits(out.cpu().numpy()), bits(rs))
        nv = norms.cpu().numpy()
        assert abs(nv[0] - np.sqrt(np.sum(rs * rs))) <= op.ndofs * U * nv[0]
        assert abs(nv[1] - op.reference_norm(b, c["u"])) <= op.ndofs * U * nv[1]


def test_device_mask_skips_and_counts_bad_facets():
    """device memory space: an id outside the mesh is skipped and counted, nothing else changes; host: refused by name"""
    import torch
    from dolfinx_eqlb_amd import cpp
    dm, mesh = setup("base")
    op = primal.PoissonOperator(mesh, 3)
    bf = mesh.boundary_facets()
    op.set_dirichlet(bf[:5])
    h = cpp.PrimalPoisson(dm, 3)
    lst = np.concatenate([bf[:5], [mesh.nfacets, -1, 2 ** 30]]).astype(np.int32)
    d_lst = torch.from_numpy(lst).to("cuda:0")
    h.set_dirichlet_raw(lst.size, d_lst.data_ptr())
    u = np.random.default_rng(0).standard_normal(op.ndofs)
    assert np.array_equal(bits(h.apply(u, masked=True)), bits(op.apply(u, masked=True)))
    _, info = h.solve(np.zeros(op.ndofs), np.zeros(op.ndofs), maxit=1)
    assert info["facets_skipped"] == 3
    with pytest.raises(RuntimeError, match=r"eqlb_primal_set_dirichlet: facets\[5\] = %d is no facet of the mesh"
                                           % mesh.nfacets):
        h.set_dirichlet(lst)
    assert np.array_equal(bits(h.apply(u, masked=True)), bits(op.apply(u, masked=True)))   # the mask as it was
    h.set_dirichlet(bf)                                                                    # a repeated call replaces
    op.set_dirichlet(bf)
    assert np.array_equal(bits(h.apply(u, masked=True)), bits(op.apply(u, masked=True)))


# ---- 2., 3. the solve against the statement's residual and a direct solve -----------------------------------------------
def check_solution(op, A, b, u0, u, info, rtol):
    """The statement's residual of u is <= tol (1 + ndofs 2^-53) (the device adds the same squares in another order);
    || u - u_direct ||_A <= tol / sqrt(lambda_min(A_ff)) + cond(A_ff) 2^-52 || u_direct ||_A: the first term from
    || e ||_A^2 = r^T A_ff^-1 r <= || r ||^2 / lambda_min, the second the accuracy of the direct solve itself."""
    assert info["converged"] == 1 and info["breakdown"] == 0
    nb = op.reference_norm(b, u0)
    assert abs(info["nb"] - nb) <= op.ndofs * U * nb
    tol = rtol * nb
    assert np.array_equal(bits(u[op.fixed]), bits(u0[op.fixed]))
    r = op.residual(b, u)
    rn = np.sqrt(np.sum(r * r))
    free = np.nonzero(~op.fixed)[0]
    Aff = A[free][:, free]
    ud = u0.copy()
    ud[free] = spla.spsolve(Aff.tocsc(), (b - A @ np.where(op.fixed, u0, 0.0))[free])
    lam = np.linalg.eigvalsh(Aff.toarray())
    e = (u - ud)[free]
    err = np.sqrt(e @ (Aff @ e))
    bound = tol / np.sqrt(lam[0]) + (lam[-1] / lam[0]) * 2.0 ** -52 * np.sqrt(ud[free] @ (Aff @ ud[free]))
    print(f"iterations {info['iterations']}, replacements {info['replacements']}, residual {rn:.3e} (tol {tol:.3e}), "
          f"energy error {err:.3e} (bound {bound:.3e}, first term {tol / np.sqrt(lam[0]):.3e})")
    assert rn <= tol * (1.0 + op.ndofs * U)
    assert abs(info["rnorm"] - rn) <= op.ndofs * U * rn
    assert err <= bound


@pytest.mark.parametrize("which", ["base", "refined"])
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_solve_dirichlet_all_around(which, p):
    c = problem(which, p)
    op, h = c["op"], c["h"]
    b = op.load(c["d"], c["f"])
    u0 = np.zeros(op.ndofs)
    u, info = h.solve(b, u0, rtol=1e-10, maxit=5000)
    A = pc.assemble(c["mesh"], p, c["kappa"])[0]
    check_solution(op, A, b, u0, u, info, 1e-10)
    # the statement's PCG takes the same number of iterations up to the rounding of the inner products
    _, si = op.pcg(b, u0, rtol=1e-10, maxit=5000)
    print(f"statement: {si['iterations']} iterations")
    assert abs(si["iterations"] - info["iterations"]) <= max(2, info["iterations"] // 20)


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_solve_mixed_boundary(p):
    """Dirichlet on two sides with inhomogeneous values, prescribed normal flux through neumann_load on the other two;
    then f = 0: nb comes from the lifting alone."""
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.eqlb.bcs import fluxbc
    dm, mesh = setup("base")
    kappa = pc.kappa_of(mesh.ncells)
    sides = gk.side_facets(mesh)
    dir_facets = np.concatenate([sides[0], sides[1]])
    op = primal.PoissonOperator(mesh, p, kappa)
    op.set_dirichlet(dir_facets)
    h = cpp.PrimalPoisson(dm, p, kappa)
    h.set_dirichlet(dir_facets)
    rng = np.random.default_rng(p)
    d = min(p, 3)
    f = rng.standard_normal(mesh.ncells * (d + 1) * (d + 2) // 2)
    be = primal.neumann_load(mesh, p, [fluxbc(lambda x, y: 1.0 + x + y * y, sides[2], scalar=True),
                                       fluxbc(lambda x, y: (np.sin(x), 2.0 + 0.0 * y), sides[3])])
    assert np.abs(be).max() > 0.0
    b = h.load(d, f, be)
    assert np.array_equal(bits(b), bits(op.load(d, f, be)))
    u0 = np.where(op.fixed, rng.standard_normal(op.ndofs), 0.0)
    start = np.where(op.fixed, u0, rng.standard_normal(op.ndofs))      # any start on the free rows
    A = pc.assemble(mesh, p, kappa)[0]
    u, info = h.solve(b, start, rtol=1e-10, maxit=5000)
    check_solution(op, A, b, u0, u, info, 1e-10)
    # f = 0 and no flux: the reference norm is that of the lifting
    zero = np.zeros(op.ndofs)
    u, info = h.solve(zero, u0, rtol=1e-10, maxit=5000)
    lift = (A @ u0)[~op.fixed]
    assert info["nb"] > 0.0 and abs(info["nb"] - np.sqrt(lift @ lift)) <= 1e-12 * info["nb"]
    check_solution(op, A, zero, u0, u, info, 1e-10)


# ---- 4. reproducibility and limits -----------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 4])
def test_reproducibility_and_limits(p):
    from dolfinx_eqlb_amd import cpp
    c = problem("base", p)
    op, h = c["op"], c["h"]
    b = op.load(c["d"], c["f"])
    u0 = np.zeros(op.ndofs)
    u1, i1 = h.solve(b, u0, rtol=1e-10, maxit=5000)
    u2, i2 = h.solve(b, u0, rtol=1e-10, maxit=5000)
    assert np.array_equal(bits(u1), bits(u2)) and i1 == i2 and i1["converged"] == 1
    # maxit = 3: the third iterate, not converged - it is the third iterate of the statement up to the rounding of
    # three steps (inner products of ndofs terms)
    u3, i3 = h.solve(b, u0, rtol=1e-10, maxit=3)
    s3, j3 = op.pcg(b, u0, rtol=1e-10, maxit=3)
    assert i3["converged"] == 0 and i3["iterations"] == 3 and i3["breakdown"] == 0 and j3["iterations"] == 3
    assert np.abs(u3 - s3).max() <= 3 * 8 * op.ndofs * U * np.abs(s3).max()
    assert abs(i3["rnorm"] - j3["rnorm"]) <= 3 * 8 * op.ndofs * U * j3["rnorm"]
    # already solved: no iteration
    u4, i4 = h.solve(b, u1, rtol=1e-9, maxit=50)
    assert i4["iterations"] == 0 and i4["converged"] == 1 and np.array_equal(bits(u4), bits(u1))
    # nothing to solve: u^
    u5, i5 = h.solve(np.zeros(op.ndofs), np.where(op.fixed, 0.0, 1.0), rtol=0.0, atol=0.0, maxit=5)
    assert i5["converged"] == 1 and i5["iterations"] == 0 and np.all(u5 == 0.0)
    # a NaN in b: breakdown within maxit
    bn = b.copy()
    bn[np.nonzero(~op.fixed)[0][7]] = np.nan
    _, i6 = h.solve(bn, u0, rtol=1e-10, maxit=40)
    assert i6["breakdown"] == 1 and i6["converged"] == 0 and i6["iterations"] <= 40
    # refusals
    h2 = cpp.PrimalPoisson(c["dm"], p)
    with pytest.raises(RuntimeError, match="singular: no Dirichlet DOF"):
        h2.solve(b, u0)
    h2.set_dirichlet(c["mesh"].boundary_facets())
    h2.set_dirichlet([])
    with pytest.raises(RuntimeError, match="singular: no Dirichlet DOF"):
        h2.solve(b, u0)
    for kw in (dict(maxit=0), dict(rtol=-1.0), dict(atol=float("nan"))):
        with pytest.raises(RuntimeError):
            h.solve(b, u0, **kw)
    with pytest.raises(RuntimeError, match="degree_dg"):
        h.load(4, c["f"])
    with pytest.raises(RuntimeError, match="p = 5"):
        cpp.PrimalPoisson(c["dm"], 5)


# ---- 5. streams ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [2])
def test_apply_and_solve_on_a_user_stream(p):
    """The inputs exist only late on the caller's non-blocking stream (behind a spin kernel; before that the buffers hold
    NaN) and are gone right behind the call: everything the calls enqueue is ordered on THAT stream."""
    import torch
    c = problem("base", p)
    op, h = c["op"], c["h"]
    b = op.load(c["d"], c["f"])
    ref_y = op.apply(c["u"], masked=True)
    ref_u, ref_info = h.solve(b, np.zeros(op.ndofs), rtol=1e-10, maxit=5000)
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    u_src, b_src = torch.from_numpy(c["u"]).to(dev), torch.from_numpy(b).to(dev)
    u_dev, b_dev = torch.full_like(u_src, float("nan")), torch.full_like(b_src, float("nan"))
    y_dev, x_dev = torch.full_like(u_src, float("nan")), torch.full_like(u_src, float("nan"))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(40_000_000)
        u_dev.copy_(u_src)
        h.apply_raw(u_dev.data_ptr(), y_dev.data_ptr(), True, stream=s.cuda_stream)
        y = y_dev.clone()
        u_dev.fill_(float("nan"))
        torch.cuda._sleep(40_000_000)
        b_dev.copy_(b_src)
        x_dev.zero_()
        info = h.solve_raw(b_dev.data_ptr(), x_dev.data_ptr(), 1e-10, 0.0, 5000, stream=s.cuda_stream)
        x = x_dev.clone()
        b_dev.fill_(float("nan"))
        x_dev.fill_(float("nan"))
    s.synchronize()
    assert np.array_equal(bits(y.cpu().numpy()), bits(ref_y))
    assert info == ref_info and np.array_equal(bits(x.cpu().numpy()), bits(ref_u))


# ---- 6. the loop ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
def test_adaptive_loop_on_the_device(oracle_mod, k):
    """project_dg, load, solve from the prolonged u, primal_flux_dg, equilibrate, estimate and oscillation,
    indicator_total, mark_doerfler(0.5), refine(keep_plan), prolong, prolong_dg and carry_boundary: three levels with
    the data of tests/test_estimator_bound.py.  Per level, with the figures of test_gpu_pipeline_bound: equilibration
    conditions, guaranteed bound against the exact error, and the estimator equal to that of the chain direct solve +
    checker + numpy estimate on the same exported mesh.  For k = 1 (and, consistently, for k = 2) the primal problem is
    solved with the projected right-hand side Pi_{k-1} f, as the equilibration needs it."""
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
    from dolfinx_eqlb_amd.eqlb import check_eqlb_conditions as chk
    from synthetic import facet_types
    import test_estimator_bound as teb
    qp, qw = make_quadrature_triangle(2 * k + 6)
    dm = cpp.DeviceMesh(create_unit_square(4, shuffle_seed=3, perturb=0.15))
    u = eq_old = ref = None
    iters = []
    for level in range(3):
        mesh = dm.mesh
        J, detJ, K = chk.cell_geometry(mesh)
        x0 = mesh.x[mesh.cell_nodes[:, 0], :2]
        xq = x0[:, None, :] + np.einsum("cij,qj->cqi", J, qp)
        fq = teb.f_ex(xq[..., 0], xq[..., 1])
        fh = cpp.project_dg(dm, k - 1, qp, qw, fq[None, :, :, None])[0]
        pp = cpp.PrimalPoisson(dm, k)
        pp.set_dirichlet(mesh.boundary_facets())
        b = pp.load(k - 1, fh)
        u, info = pp.solve(b, np.zeros(pp.ndofs) if u is None else u, rtol=1e-12, maxit=5000)
        assert info["converged"] == 1
        iters.append(info["iterations"])
        cd, ndofs = dm.lagrange_dofmap(k)
        G = cpp.primal_flux_dg(dm, k, k - 1, cd, u)[0]
        eq = cpp.SemiExplicitEquilibrator(dm, k, 1)
        if level == 0:
            eq.set_boundary(facet_types(mesh, None))
        else:
            eq.carry_boundary(eq_old, ref)
        x = eq.equilibrate_host(G[None], fh[None])
        div2, sig2, jump = cpp.estimate(dm, k, x, G[None], fh[None])
        eta_osc2 = cpp.oscillation(dm, k, x, G[None], qp, qw, fq[None])[0]
        cell_eta2, totals = cpp.indicator_total([sig2[0], eta_osc2], pair_last_two=True)
        eta = float(np.sqrt(totals[-1]))
        # the figures
        gcd = gk.dofmap(mesh, k)[0]
        assert np.array_equal(gcd, cd)
        err = gk.energy_error(mesh, k, u, gcd, teb.grad_ex)
        fh_ref, osc2, hc = gk.project_rhs(mesh, k, teb.f_ex)
        u_ref, _ = gk.solve_poisson(mesh, k, teb.f_ex, f_dg=fh_ref)
        G_ref = gk.discrete_flux(mesh, k, u_ref, gcd)
        x_ref = oracle_mod.se_reconstruct(mesh, k, facet_types(mesh, None), G_ref[None], fh_ref[None])[0]
        eta_ref = teb.estimate(teb.flux_norm2(mesh, k, x_ref), osc2, hc)
        print(f"k={k} level {level}: {mesh.ncells} cells, {info['iterations']} iterations, eta {eta:.6e}, "
              f"eta_ref {eta_ref:.6e}, err {err:.6e}, effectivity {eta / err:.4f}")
        assert np.sqrt(div2.sum()) < 1e-9 * np.sqrt(np.sum(fh ** 2)) and jump.max() < 1e-9
        assert eta / err >= 1.0 - 1e-10
        assert abs(eta - eta_ref) <= 1e-9 * eta
        if level == 2:
            break
        marked, _ = cpp.mark_doerfler(cell_eta2, 0.5)
        ref = dm.refine(marked, keep_plan=True)
        u = ref.prolong(k, u)
        fh2 = ref.prolong_dg(k - 1, fh)
        assert u.size == ref.dmesh.lagrange_dofmap(k)[1] and np.isfinite(fh2).all()
        eq_old, dm_old, dm = eq, dm, ref.dmesh
        _CACHE[("loop", k, level)] = (dm_old, eq_old, ref)   # the plan reads the old handles: they outlive the level
    print(f"k={k}: iterations per level {iters}")
