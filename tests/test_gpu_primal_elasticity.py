"""The P_p^2 elasticity solve on the device (cpp.PrimalElasticity, csrc/eqlb_primal_elasticity.hip) against its numpy
statement (dolfinx_eqlb_amd/lsolver/primal.py: ElasticityOperator): operator, load, diagonal and residual bit for bit;
the CG against the statement's residual and a direct solve, with derived bounds; the limits of the iteration; a caller's
stream; and the adaptive loop of the reference's demo_cook.py closed on the device.

The base mesh create_unit_square(9, shuffle_seed=3, perturb=0.15) has 324 cells, that of tests/test_gpu_primal_solve.py.
The cell kernel takes 128 cells per workgroup: 324 cells are two full workgroups and a last one of 68 cells, so the mesh
exercises the hand-over between workgroups and the partial last one; the sum pass and the vector kernels take 256 rows
per block and see 2 ndofs >= 380 rows, more than one block, with a partial last one.  The mesh is also used refined once
on the device at refine_cases.level_marks.  pi_1 is log-uniform in [0.5, 50] per cell (elasticity_cases.pi1_of)."""

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import elasticity_cases as ec
import galerkin as gk
from dolfinx_eqlb_amd.lsolver import primal
from dolfinx_eqlb_amd.mesh import create_unit_square

pytestmark = pytest.mark.gpu

U = ec.U
_CACHE = {}
MIXED = [(True, False), (False, True), (True, True)]   # side 3 and the rows not named: Dirichlet


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
    """the statement, the handle and the data of one (mesh, p), computed once: Dirichlet all around in both rows"""
    key = (which, p)
    if key not in _CACHE:
        from dolfinx_eqlb_amd import cpp
        dm, mesh = setup(which)
        rng = np.random.default_rng(17 * p + len(which))
        pi = ec.pi1_of(mesh.ncells)
        lists = ec.dirichlet_lists(gk.elasticity_facet_types(mesh, []))
        op = primal.ElasticityOperator(mesh, p, cell_pi1=pi)
        op.set_dirichlet(*lists)
        d = min(p, 3)
        n = 2 * op.ndofs
        f = rng.standard_normal((2, mesh.ncells * (d + 1) * (d + 2) // 2))
        e = rng.standard_normal(n)
        u = rng.standard_normal(n)
        h = cpp.PrimalElasticity(dm, p, cell_pi1=pi)
        h.set_dirichlet(*lists)
        assert h.ndofs == op.ndofs
        _CACHE[key] = dict(dm=dm, mesh=mesh, pi=pi, op=op, h=h, d=d, f=f, e=e, u=u, n=n, b=op.load(d, f, e),
                           lists=lists)
    return _CACHE[key]


# ---- 1. bit for bit --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["base", "refined"])
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_statements_bit_for_bit_host_memory(which, p):
    c = problem(which, p)
    op, h, u, b, n = c["op"], c["h"], c["u"], c["b"], c["n"]
    for call in range(2):   # a second call gives the same bits
        assert np.array_equal(bits(h.apply(u)), bits(op.apply(u)))
        assert np.array_equal(bits(h.apply(u, masked=True)), bits(op.apply(u, masked=True)))
        assert np.array_equal(bits(h.load(c["d"], c["f"])), bits(op.load(c["d"], c["f"])))
        assert np.array_equal(bits(h.load(c["d"], c["f"], c["e"])), bits(b))
        assert np.array_equal(bits(h.diagonal()), bits(op.diagonal()))
        r, rn, nb = h.residual(b, u, norms=True)
        rs = op.residual(b, u)
        assert np.array_equal(bits(r), bits(rs))
        # the norms are sums in another order: 2 ndofs roundings
        assert abs(rn - np.sqrt(np.sum(rs * rs))) <= n * U * rn
        assert abs(nb - op.reference_norm(b, u)) <= n * U * nb
        assert np.array_equal(bits(h.residual(b, u)), bits(rs))


@pytest.mark.parametrize("which", ["base", "refined"])
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_statements_bit_for_bit_device_memory(which, p):
    import torch
    from dolfinx_eqlb_amd import cpp
    c = problem(which, p)
    op, h, b, n = c["op"], c["h"], c["b"], c["n"]
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    u, bb, f, e = t(c["u"]), t(b), t(c["f"]), t(c["e"])
    out = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    norms = torch.full((2,), float("nan"), dtype=torch.float64, device=dev)
    # a handle made and masked from device memory computes the same
    pi_d, l0, l1 = t(c["pi"]), t(c["lists"][0]), t(c["lists"][1])
    torch.cuda.synchronize()
    h2 = cpp.PrimalElasticity.create_raw(c["dm"], p, 1.0, pi_d.data_ptr())
    h2.set_dirichlet_raw(l0.numel(), l0.data_ptr(), l1.numel(), l1.data_ptr())
    for handle in (h, h2):
        for call in range(2):
            handle.apply_raw(u.data_ptr(), out.data_ptr(), False)
            assert np.array_equal(bits(out.cpu().numpy()), bits(op.apply(c["u"])))
            handle.apply_raw(u.data_ptr(), out.data_ptr(), True)
            assert np.array_equal(bits(out.cpu().numpy()), bits(op.apply(c["u"], masked=True)))
            handle.load_raw(c["d"], f.data_ptr(), e.data_ptr(), out.data_ptr())
            assert np.array_equal(bits(out.cpu().numpy()), bits(b))
            handle.load_raw(c["d"], f.data_ptr(), None, out.data_ptr())
            assert np.array_equal(bits(out.cpu().numpy()), bits(op.load(c["d"], c["f"])))
            handle.diagonal_raw(out.data_ptr())
            assert np.array_equal(bits(out.cpu().numpy()), bits(op.diagonal()))
            handle.residual_raw(bb.data_ptr(), u.data_ptr(), out.data_ptr(), norms.data_ptr())
            rs = op.residual(b, c["u"])
            assert np.array_equal(bits(out.cpu().numpy()), bits(rs))
            nv = norms.cpu().numpy()
            assert abs(nv[0] - np.sqrt(np.sum(rs * rs))) <= n * U * nv[0]
            assert abs(nv[1] - op.reference_norm(b, c["u"])) <= n * U * nv[1]


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_scalar_pi_1_bit_for_bit(p):
    """the scalar pi_1 of a handle without cell_pi1, masked per component by a mixed layout"""
    from dolfinx_eqlb_amd import cpp
    dm, mesh = setup("base")
    lists = ec.dirichlet_lists(gk.elasticity_facet_types(mesh, MIXED))
    op = primal.ElasticityOperator(mesh, p, 7.25)
    op.set_dirichlet(*lists)
    h = cpp.PrimalElasticity(dm, p, 7.25)
    h.set_dirichlet(*lists)
    u = np.random.default_rng(p).standard_normal(2 * op.ndofs)
    assert not np.array_equal(op.fixed[0::2], op.fixed[1::2])
    assert np.array_equal(bits(h.apply(u, masked=True)), bits(op.apply(u, masked=True)))
    assert np.array_equal(bits(h.diagonal()), bits(op.diagonal()))
    assert np.array_equal(bits(h.residual(u[::-1], u)), bits(op.residual(u[::-1], u)))


# ---- 2. the mask on the device -----------------------------------------------------------------------------------------
def test_device_mask_skips_and_counts_bad_facets():
    """device memory space: an id outside the mesh, in either list, is skipped and counted, nothing else changes; host:
    refused by name, the mask as it was"""
    import torch
    from dolfinx_eqlb_amd import cpp
    dm, mesh = setup("base")
    op = primal.ElasticityOperator(mesh, 3)
    bf = mesh.boundary_facets()
    op.set_dirichlet(bf[:5], bf[3:9])
    h = cpp.PrimalElasticity(dm, 3)
    l0 = np.concatenate([bf[:5], [mesh.nfacets, -1]]).astype(np.int32)
    l1 = np.concatenate([[2 ** 30], bf[3:9]]).astype(np.int32)
    d0, d1 = torch.from_numpy(l0).to("cuda:0"), torch.from_numpy(l1).to("cuda:0")
    h.set_dirichlet_raw(l0.size, d0.data_ptr(), l1.size, d1.data_ptr())
    n = 2 * op.ndofs
    u = np.random.default_rng(0).standard_normal(n)
    assert np.array_equal(bits(h.apply(u, masked=True)), bits(op.apply(u, masked=True)))
    _, info = h.solve(np.zeros(n), np.zeros(n), maxit=1)
    assert info["facets_skipped"] == 3
    with pytest.raises(RuntimeError, match=r"facets0\[5\] = %d is no facet of the mesh" % mesh.nfacets):
        h.set_dirichlet(l0, bf)
    with pytest.raises(RuntimeError, match=r"facets1\[0\] = %d is no facet of the mesh" % 2 ** 30):
        h.set_dirichlet(bf, l1)
    assert np.array_equal(bits(h.apply(u, masked=True)), bits(op.apply(u, masked=True)))   # the mask as it was
    h.set_dirichlet(bf, bf[:2])                                                            # a repeated call replaces
    op.set_dirichlet(bf, bf[:2])
    assert np.array_equal(bits(h.apply(u, masked=True)), bits(op.apply(u, masked=True)))


# ---- 3. the solve against the statement's residual and a direct solve ---------------------------------------------------
def extreme_eigenvalues(Aff):
    """(lambda_min, lambda_max) of the SPD matrix: dense up to 3000 rows; above (p = 4 on the base mesh: 5 000 rows,
    half a minute dense) the two extreme ones from scipy.sparse.linalg.eigsh - the largest by Lanczos, the smallest by
    shift-and-invert at 0 - each converged to 1e-10 relative."""
    if Aff.shape[0] <= 3000:
        lam = np.linalg.eigvalsh(Aff.toarray())
        return lam[0], lam[-1]
    hi = spla.eigsh(Aff, k=1, which="LA", tol=1e-10, return_eigenvectors=False)[0]
    lo = spla.eigsh(Aff.tocsc(), k=1, sigma=0.0, which="LM", tol=1e-10, return_eigenvectors=False)[0]
    return lo, hi


def check_solution(op, A, b, u0, u, info, rtol):
    """check_solution of tests/test_gpu_primal_solve.py with n = 2 ndofs rows.  The statement's residual of u is
    <= tol (1 + n 2^-53) (the device adds the same squares in another order); || u - u_direct ||_A <= tol /
    sqrt(lambda_min(A_ff)) + cond(A_ff) 2^-52 || u_direct ||_A: the first term from || e ||_A^2 = r^T A_ff^-1 r
    <= || r ||^2 / lambda_min, the second the accuracy of the direct solve itself."""
    n = 2 * op.ndofs
    assert info["converged"] == 1 and info["breakdown"] == 0
    nb = op.reference_norm(b, u0)
    assert abs(info["nb"] - nb) <= n * U * nb
    tol = rtol * nb
    assert np.array_equal(bits(u[op.fixed]), bits(u0[op.fixed]))
    r = op.residual(b, u)
    rn = np.sqrt(np.sum(r * r))
    free = np.nonzero(~op.fixed)[0]
    Aff = A[free][:, free]
    ud = u0.copy()
    ud[free] = spla.spsolve(Aff.tocsc(), (b - A @ np.where(op.fixed, u0, 0.0))[free])
    lo, hi = extreme_eigenvalues(Aff)
    e = (u - ud)[free]
    err = np.sqrt(e @ (Aff @ e))
    bound = tol / np.sqrt(lo) + (hi / lo) * 2.0 ** -52 * np.sqrt(ud[free] @ (Aff @ ud[free]))
    print(f"iterations {info['iterations']}, replacements {info['replacements']}, residual {rn:.3e} (tol {tol:.3e}), "
          f"energy error {err:.3e} (bound {bound:.3e}, first term {tol / np.sqrt(lo):.3e})")
    assert rn <= tol * (1.0 + n * U)
    assert abs(info["rnorm"] - rn) <= n * U * rn
    assert err <= bound
    return ud


@pytest.mark.parametrize("which,p", [("base", 1), ("base", 2), ("base", 3), ("base", 4), ("refined", 1), ("refined", 2)])
def test_solve_dirichlet_all_around(which, p):
    c = problem(which, p)
    op, h, n = c["op"], c["h"], c["n"]
    b = op.load(c["d"], c["f"])
    u0 = np.zeros(n)
    u, info = h.solve(b, u0, rtol=1e-10, maxit=20000)
    A = ec.assemble(c["mesh"], p, 1.0, c["pi"])[0]
    check_solution(op, A, b, u0, u, info, 1e-10)
    # the statement's PCG takes the same number of iterations up to the rounding of the inner products
    _, si = op.pcg(b, u0, rtol=1e-10, maxit=20000)
    print(f"statement: {si['iterations']} iterations")
    assert abs(si["iterations"] - info["iterations"]) <= max(2, info["iterations"] // 20)


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_solve_mixed_boundary(p):
    """galerkin.elasticity_facet_types(MIXED): tractions in row 0 on side 0, in row 1 on side 1, in both rows on side
    2, through traction_load; inhomogeneous Dirichlet values on the other rows; any start on the free rows."""
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.eqlb.bcs import fluxbc
    dm, mesh = setup("base")
    pi = ec.pi1_of(mesh.ncells)
    ft = gk.elasticity_facet_types(mesh, MIXED)
    lists = ec.dirichlet_lists(ft)
    op = primal.ElasticityOperator(mesh, p, cell_pi1=pi)
    op.set_dirichlet(*lists)
    h = cpp.PrimalElasticity(dm, p, cell_pi1=pi)
    h.set_dirichlet(*lists)
    rng = np.random.default_rng(p)
    d = min(p, 3)
    n = 2 * op.ndofs
    f = rng.standard_normal((2, mesh.ncells * (d + 1) * (d + 2) // 2))
    g = [lambda x, y: 1.0 + x + y * y, lambda x, y: np.sin(x) - 2.0 * y]       # the normal fluxes -t_r of the rows
    be = primal.traction_load(mesh, p, [[fluxbc(g[r], np.nonzero(ft[r] == 2)[0], scalar=True)] for r in range(2)])
    assert np.abs(be[0::2]).max() > 0.0 and np.abs(be[1::2]).max() > 0.0
    b = h.load(d, f, be)
    assert np.array_equal(bits(b), bits(op.load(d, f, be)))
    u0 = np.where(op.fixed, rng.standard_normal(n), 0.0)
    start = np.where(op.fixed, u0, rng.standard_normal(n))
    A = ec.assemble(mesh, p, 1.0, pi)[0]
    u, info = h.solve(b, start, rtol=1e-10, maxit=20000)
    check_solution(op, A, b, u0, u, info, 1e-10)


# ---- 4. reproducibility and limits -----------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 4])
def test_reproducibility_and_limits(p):
    from dolfinx_eqlb_amd import cpp
    c = problem("base", p)
    op, h, n = c["op"], c["h"], c["n"]
    b = op.load(c["d"], c["f"])
    u0 = np.zeros(n)
    u1, i1 = h.solve(b, u0, rtol=1e-10, maxit=20000)
    u2, i2 = h.solve(b, u0, rtol=1e-10, maxit=20000)
    assert np.array_equal(bits(u1), bits(u2)) and i1 == i2 and i1["converged"] == 1
    # maxit = 3: the third iterate, not converged - it is the third iterate of the statement up to the rounding of
    # three steps (inner products of 2 ndofs terms)
    u3, i3 = h.solve(b, u0, rtol=1e-10, maxit=3)
    s3, j3 = op.pcg(b, u0, rtol=1e-10, maxit=3)
    assert i3["converged"] == 0 and i3["iterations"] == 3 and i3["breakdown"] == 0 and j3["iterations"] == 3
    assert np.abs(u3 - s3).max() <= 3 * 8 * n * U * np.abs(s3).max()
    assert abs(i3["rnorm"] - j3["rnorm"]) <= 3 * 8 * n * U * j3["rnorm"]
    # already solved: no iteration
    u4, i4 = h.solve(b, u1, rtol=1e-9, maxit=50)
    assert i4["iterations"] == 0 and i4["converged"] == 1 and np.array_equal(bits(u4), bits(u1))
    # nothing to solve: u^
    u5, i5 = h.solve(np.zeros(n), np.where(op.fixed, 0.0, 1.0), rtol=0.0, atol=0.0, maxit=5)
    assert i5["converged"] == 1 and i5["iterations"] == 0 and np.all(u5 == 0.0)
    # a NaN in b: breakdown within maxit
    bn = b.copy()
    bn[np.nonzero(~op.fixed)[0][7]] = np.nan
    _, i6 = h.solve(bn, u0, rtol=1e-10, maxit=40)
    assert i6["breakdown"] == 1 and i6["converged"] == 0 and i6["iterations"] <= 40
    # refusals: one per component
    bf = c["mesh"].boundary_facets()
    h2 = cpp.PrimalElasticity(c["dm"], p)
    with pytest.raises(RuntimeError, match="singular: component 0 has no Dirichlet DOF"):
        h2.solve(b, u0)
    h2.set_dirichlet(bf, [])
    with pytest.raises(RuntimeError, match="singular: component 1 has no Dirichlet DOF"):
        h2.solve(b, u0)
    h2.set_dirichlet([], bf)
    with pytest.raises(RuntimeError, match="singular: component 0 has no Dirichlet DOF"):
        h2.solve(b, u0)
    for kw in (dict(maxit=0), dict(rtol=-1.0), dict(atol=float("nan"))):
        with pytest.raises(RuntimeError):
            h.solve(b, u0, **kw)
    with pytest.raises(RuntimeError, match="degree_dg"):
        h.load(4, c["f"])
    with pytest.raises(RuntimeError, match="p = 5"):
        cpp.PrimalElasticity(c["dm"], 5)


# ---- 5. streams ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [2])
def test_apply_and_solve_on_a_user_stream(p):
    """The inputs exist only late on the caller's non-blocking stream (behind a spin kernel; before that the buffers hold
    NaN) and are gone right behind the call: everything the calls enqueue is ordered on THAT stream."""
    import torch
    c = problem("base", p)
    op, h, n = c["op"], c["h"], c["n"]
    b = op.load(c["d"], c["f"])
    ref_y = op.apply(c["u"], masked=True)
    ref_u, ref_info = h.solve(b, np.zeros(n), rtol=1e-10, maxit=20000)
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
        info = h.solve_raw(b_dev.data_ptr(), x_dev.data_ptr(), 1e-10, 0.0, 20000, stream=s.cuda_stream)
        x = x_dev.clone()
        b_dev.fill_(float("nan"))
        x_dev.fill_(float("nan"))
    s.synchronize()
    assert np.array_equal(bits(y.cpu().numpy()), bits(ref_y))
    assert info == ref_info and np.array_equal(bits(x.cpu().numpy()), bits(ref_u))


# ---- 6. the loop ------------------------------------------------------------------------------------------------------
def test_adaptive_loop_on_the_device():
    """k = 2, three levels from create_unit_square(4, shuffle_seed=3, perturb=0.15), layout [(True, True)]: tractions
    on side 0 in both rows, u = 0 elsewhere.  Per level: project_dg of the body force, load + traction_load, solve from
    the prolonged u, primal_stress_dg, the stress equilibrator (set_boundary and update_flux_bc on level 0,
    carry_boundary after), kornconst_host, estimate_stress, indicator_total, mark_doerfler(0.5), refine(keep_plan),
    prolong(bs=2).  The tractions are affine along the side, so the facet DOFs the equilibrator holds (moments up to
    k - 1) and carries across a bisection are those of the traction itself on every level, as the load has it.  The
    same `fluxbc` callables - the normal fluxes -t_r of the rows - feed traction_load and the equilibrator: that the
    divergence condition holds at rounding level on the boundary patches checks the sign of traction_load."""
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_interval, make_quadrature_triangle
    from dolfinx_eqlb_amd.eqlb import check_eqlb_conditions as chk
    from dolfinx_eqlb_amd.eqlb.bcs import fluxbc
    k, pi_1, layout = 2, 2.0, [(True, True)]
    g = [lambda x, y: -(0.3 + 0.5 * y) + 0.0 * x, lambda x, y: -(0.2 - 0.4 * y) + 0.0 * x]   # -t_r on x = 0
    force = [lambda x, y: np.sin(2.0 * x + y), lambda x, y: 1.0 + x * y]
    qp, qw = make_quadrature_triangle(2 * k + 6)
    s, ws = make_quadrature_interval(2 * k)
    dm = cpp.DeviceMesh(create_unit_square(4, shuffle_seed=3, perturb=0.15))
    u = eq_old = ref = None
    iters = []
    for level in range(3):
        mesh = dm.mesh
        J, detJ, K = chk.cell_geometry(mesh)
        x0 = mesh.x[mesh.cell_nodes[:, 0], :2]
        xq = x0[:, None, :] + np.einsum("cij,qj->cqi", J, qp)
        fq = np.stack([fn(xq[..., 0], xq[..., 1]) for fn in force])
        fh = cpp.project_dg(dm, k - 1, qp, qw, fq[:, :, :, None])
        ft = gk.elasticity_facet_types(mesh, layout)
        lists = ec.dirichlet_lists(ft)
        side0 = gk.side_facets(mesh)[0].astype(np.int32)
        assert all(np.array_equal(np.nonzero(ft[r] == 2)[0], np.sort(side0)) for r in range(2))
        rows = [[fluxbc(g[r], side0, scalar=True)] for r in range(2)]
        el = cpp.PrimalElasticity(dm, k, pi_1)
        el.set_dirichlet(*lists)
        n = 2 * el.ndofs
        b = el.load(k - 1, fh, primal.traction_load(mesh, k, rows))
        start = np.zeros(n) if u is None else u
        u, info = el.solve(b, start, rtol=1e-12, maxit=20000)
        assert info["converged"] == 1
        iters.append(info["iterations"])
        # the direct solve of the assembled system on the exported mesh, within check_solution's bound
        op = primal.ElasticityOperator(mesh, k, pi_1)
        op.set_dirichlet(*lists)
        assert np.array_equal(bits(b), bits(op.load(k - 1, fh, primal.traction_load(mesh, k, rows))))
        u_ref = check_solution(op, ec.assemble(mesh, k, pi_1)[0], b, np.where(op.fixed, start, 0.0), u, info, 1e-12)
        cd, ndofs = dm.lagrange_dofmap(k)
        assert ndofs == el.ndofs
        eq = cpp.SemiExplicitEquilibrator(dm, k, 2, reconstruct_stress=True, estimate_korn=True)
        if level == 0:
            eq.set_boundary(ft)
            xs = cpp.facet_points(dm, side0, s)
            for r in range(2):
                eq.update_flux_bc(r, side0, g[r](xs[..., 0], xs[..., 1]), s, ws)
        else:
            eq.carry_boundary(eq_old, ref)
        korn = np.sqrt(eq.kornconst_host())

        def chain(uu):
            G = cpp.primal_stress_dg(dm, k, k - 1, cd, uu, pi_1=pi_1)
            x = eq.equilibrate_host(G, fh)
            energy, wsym, _ = cpp.estimate_stress(dm, k, x, korn, pi_1)
            cell_eta2, totals = cpp.indicator_total([energy, wsym])
            return G, x, cell_eta2, float(np.sqrt(totals[-1]))

        G, x, cell_eta2, eta = chain(u)
        eta_ref = chain(u_ref)[3]
        div2, _, jump = cpp.estimate(dm, k, x, G, fh)
        print(f"level {level}: {mesh.ncells} cells, {info['iterations']} iterations, eta {eta:.6e}, "
              f"eta_ref {eta_ref:.6e}, div {np.sqrt(div2.sum()):.2e}, jump {jump.max():.2e}")
        assert np.sqrt(div2.sum()) < 1e-9 * np.sqrt(np.sum(fh ** 2)) and jump.max() < 1e-9
        assert eta > 0.0 and abs(eta - eta_ref) <= 1e-9 * eta
        if level == 2:
            break
        marked, _ = cpp.mark_doerfler(cell_eta2, 0.5)
        ref = dm.refine(marked, keep_plan=True)
        u = ref.prolong(k, u, bs=2)
        assert u.size == 2 * ref.dmesh.lagrange_dofmap(k)[1]
        eq_old, dm_old, dm = eq, dm, ref.dmesh
        _CACHE[("loop", level)] = (dm_old, eq_old, ref)   # the plan reads the old handles: they outlive the level
    print(f"iterations per level {iters}")
    assert iters[0] > 0
