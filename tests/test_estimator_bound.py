"""End-to-end validation with REAL discrete solutions (the reference's demos and convergence
tests, demo/poisson/demo_error_estimation.py:52-124, python/test/unit/test_fluxeqlb_convrate.py:
131-135): P_k Galerkin solve -> sigma_h = -grad u_h -> equilibration -> the Prager-Synge estimate
    || grad(u - u_h) || <= || sigma_eq || + (h/pi) || f - Pi f ||
must be a guaranteed upper bound with an effectivity index close to one, and
|| div(sigma_eq + sigma_h) - f || must converge with order k.  A wrong sign or orientation
convention anywhere in the chain breaks the bound."""

import numpy as np
import pytest

import galerkin as gk
from dolfinx_eqlb_amd.eqlb import check_eqlb_conditions as chk
from dolfinx_eqlb_amd.mesh import create_unit_square
from synthetic import facet_types


def u_ex(x, y):
    return np.sin(np.pi * x) * np.sin(np.pi * y) * (1.0 + x)


def grad_ex(x, y):
    s, c = np.sin, np.cos
    return (np.pi * c(np.pi * x) * s(np.pi * y) * (1 + x) + s(np.pi * x) * s(np.pi * y),
            np.pi * s(np.pi * x) * c(np.pi * y) * (1 + x))


def f_ex(x, y):
    s, c = np.sin, np.cos
    return 2 * np.pi ** 2 * s(np.pi * x) * s(np.pi * y) * (1 + x) - 2 * np.pi * c(np.pi * x) * s(np.pi * y)


def problem(n, k, shuffle=3):
    mesh = create_unit_square(n, shuffle_seed=shuffle, perturb=0.15)
    fh, osc2, h = gk.project_rhs(mesh, k, f_ex)
    u, cd = gk.solve_poisson(mesh, k, f_ex, f_dg=fh if k == 1 else None)
    G = gk.discrete_flux(mesh, k, u, cd)
    err = gk.energy_error(mesh, k, u, cd, grad_ex)
    return mesh, facet_types(mesh, None), G, fh, osc2, h, err


def flux_norm2(mesh, k, x):
    from test_gpu_estimate import flux_norm2_cells
    return flux_norm2_cells(mesh, k, x)


def estimate(eta_sig2, osc2, h):
    eta_osc2 = (h / np.pi) ** 2 * osc2
    return float(np.sqrt(np.sum(eta_sig2 + eta_osc2 + 2 * np.sqrt(eta_sig2 * eta_osc2))))


@pytest.mark.parametrize("k", [1, 2, 3])
def test_guaranteed_upper_bound_and_rates(oracle_mod, k):
    eff, errs, hdiv = [], [], []
    ns = (4, 8, 16)
    for n in ns:
        mesh, ft, G, fh, osc2, h, err = problem(n, k)
        x = oracle_mod.se_reconstruct(mesh, k, ft, G[None], fh[None])[0]
        res, nrm = chk.divergence_residual(mesh, k, x, G, fh)
        assert res < 1e-9 * nrm and chk.check_jump_condition(mesh, k, x, G, atol=1e-9)
        eta = estimate(flux_norm2(mesh, k, x), osc2, h)
        eff.append(eta / err)
        errs.append(err)
        hdiv.append(chk.hdiv_seminorm_error(mesh, k, x, G, f_ex))
    assert all(e >= 1.0 - 1e-10 for e in eff), eff          # guaranteed bound
    assert eff[-1] < 1.6, eff                                # and a sharp one
    rate_err = np.log2(errs[-2] / errs[-1])
    rate_div = np.log2(hdiv[-2] / hdiv[-1])
    assert rate_err > k - 0.2 and rate_div > k - 0.1, (rate_err, rate_div)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 3])
def test_gpu_pipeline_bound(k):
    """Same chain on the device: projector -> equilibration -> eqlb_se_estimate."""
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
    mesh, ft, G, fh, osc2, h, err = problem(12, k)
    dm = cpp.DeviceMesh(mesh)
    # the projected right-hand side from point values, on the device
    qp, qw = make_quadrature_triangle(2 * k + 6)
    J, detJ, K = chk.cell_geometry(mesh)
    x0 = mesh.x[mesh.cell_nodes[:, 0], :2]
    xq = x0[:, None, :] + np.einsum("cij,qj->cqi", J, qp)
    fh_dev = cpp.project_dg(dm, k - 1, qp, qw, f_ex(xq[..., 0], xq[..., 1])[None, :, :, None])[0]
    assert np.allclose(fh_dev, fh, rtol=1e-10, atol=1e-10)
    eq = cpp.SemiExplicitEquilibrator(dm, k, 1)
    eq.set_boundary(ft)
    x = eq.equilibrate_host(G[None], fh_dev[None])
    div2, sig2, jump = cpp.estimate(dm, k, x, G[None], fh_dev[None])
    assert np.sqrt(div2.sum()) < 1e-9 * np.sqrt(np.sum(fh ** 2)) and jump.max() < 1e-9
    eta = estimate(sig2[0], osc2, h)
    assert 1.0 - 1e-10 <= eta / err < 1.6
    # the oscillation term from the device as well (eqlb_oscillation: exact f at the quadrature points,
    # div(sigma_eq + G) evaluated exactly): the whole estimator of demo_error_estimation.py:93-120
    eta_osc2 = cpp.oscillation(dm, k, x, G[None], qp, qw, f_ex(xq[..., 0], xq[..., 1])[None])[0]
    assert np.allclose(eta_osc2, (h / np.pi) ** 2 * osc2, rtol=1e-8, atol=1e-12 * eta_osc2.max())
    eta_dev = float(np.sqrt(np.sum(sig2[0] + eta_osc2 + 2 * np.sqrt(sig2[0] * eta_osc2))))
    assert abs(eta_dev - eta) <= 1e-9 * eta


def ev_flux_error2(mesh, k, xb, G):
    """|| sigma_EV - G ||^2_T per cell (err_sig = grad(u_h) + sigma_eqlb of the reference's
    estimator for a conforming flux, demo_error_estimation.py:97-100), xb: broken coefficients."""
    from dolfinx_eqlb_amd.elmtlib import e_raviart_thomas as ert
    from dolfinx_eqlb_amd.elmtlib.lagrange import Lagrange
    from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
    J, detJ, K = chk.cell_geometry(mesh)
    rt = ert.HierarchicRT(k)
    dg = Lagrange(k - 1)
    qp, qw = make_quadrature_triangle(2 * k + 2)
    phi = rt.tabulate(qp)
    c = xb.reshape(mesh.ncells, rt.ndofs)
    sig = np.einsum("cdX,ci,qiX->cqd", J, c, phi) / detJ[:, None, None]
    Gq = np.einsum("cjd,qj->cqd", G.reshape(mesh.ncells, dg.ndofs, 2), dg.tabulate(qp)[0])
    return np.einsum("q,cqd,cqd->c", qw, sig - Gq, sig - Gq) * np.abs(detJ)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_ev_guaranteed_upper_bound(oracle_mod, k):
    """The constrained-minimisation flux gives a guaranteed bound as well.  With the flux degree
    equal to the primal degree it is less sharp than the semi-explicit flux for k >= 2 (hat_a G is
    a P_k field that RT_k does not contain; measured effectivity at n = 4/8/16: k = 2
    1.30/1.34/1.51, k = 3 1.36/1.71/2.75 on the flux part), so only the bound is asserted tightly."""
    from dolfinx_eqlb_amd.eqlb.conforming import conforming_dofmap, conforming_to_broken
    mesh, ft, G, fh, osc2, h, err = problem(8, k)
    cd, nd = conforming_dofmap(mesh, k)
    x = oracle_mod.ev_reconstruct(mesh, k, ft, G[None], fh[None], cd, nd)[0]
    xb = conforming_to_broken(mesh, k, x)
    res, nrm = chk.divergence_residual(mesh, k, xb, np.zeros_like(G), fh)
    assert res < 1e-9 * nrm
    eta_ev = estimate(ev_flux_error2(mesh, k, xb, G), osc2, h)
    xs = oracle_mod.se_reconstruct(mesh, k, ft, G[None], fh[None])[0]
    eta_se = estimate(flux_norm2(mesh, k, xs), osc2, h)
    assert 1.0 - 1e-10 <= eta_ev / err < 2.0
    assert eta_ev < 1.5 * eta_se


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 3])
def test_gpu_ev_pipeline_bound(k):
    """EV on the device: equilibrate (broken output) -> eqlb_ev_estimate; guaranteed bound."""
    from dolfinx_eqlb_amd import cpp
    mesh, ft, G, fh, osc2, h, err = problem(10, k)
    dm = cpp.DeviceMesh(mesh)
    ev = cpp.ConstrainedMinEquilibrator(dm, k, 1)
    ev.set_option("output", 1)
    ev.set_boundary(ft)
    xb = ev.equilibrate_host(G[None], fh[None])
    div2, sig2, jump = cpp.estimate(dm, k, xb, G[None], fh[None], conforming_flux=True)
    assert np.sqrt(div2.sum()) < 1e-9 * np.sqrt(np.sum(fh ** 2)) and jump.max() < 1e-9
    ref = ev_flux_error2(mesh, k, xb[0], G)
    # || sigma - G ||^2 is evaluated as (sigma, sigma) - 2 (sigma, G) + (G, G): the difference of
    # O(|G|^2 |T|) terms, so the tolerance is relative to that scale
    scale = np.abs(G).max() ** 2 * np.abs(chk.cell_geometry(mesh)[1]).max()
    assert np.allclose(sig2[0], ref, rtol=1e-6, atol=1e-13 * scale)
    eta = estimate(sig2[0], osc2, h)
    assert 1.0 - 1e-10 <= eta / err < 2.2


# ---- linear elasticity: the estimate of the reference's demo/elasticity/demo_error_estimation.py:49-148 against a true
# error.  -div(2 eps(u) + pi_1 div(u) I) = f on the unit square, u = 0 all around, with the exact solution
# u = (sin(pi x) sin(pi y) (1 + x), sin(2 pi x) sin(pi y) e^y): it vanishes on the boundary, so no boundary data error
# enters the bound.
_EXACT = {}


def elasticity_exact():
    """(u, grad u, f): callables (x, y[, pi_1]) -> arrays [2, ...], [2, 2, ...] (gu[r][d] = d_d u_r), [2, ...]; f from the
    exact derivatives (sympy)."""
    if not _EXACT:
        import sympy as sy
        x, y, p = sy.symbols("x y pi_1")
        u = [sy.sin(sy.pi * x) * sy.sin(sy.pi * y) * (1 + x), sy.sin(2 * sy.pi * x) * sy.sin(sy.pi * y) * sy.exp(y)]
        gu = [[sy.diff(u[r], v) for v in (x, y)] for r in range(2)]
        div = gu[0][0] + gu[1][1]
        sig = [[gu[r][d] + gu[d][r] + (p * div if r == d else 0) for d in range(2)] for r in range(2)]
        f = [-(sy.diff(sig[r][0], x) + sy.diff(sig[r][1], y)) for r in range(2)]

        def fn(expr, args):
            g = sy.lambdify(args, expr, "numpy")
            return lambda *a: g(*a) + 0.0 * a[0]              # a constant expression still gives an array
        _EXACT["u"] = [fn(e, (x, y)) for e in u]
        _EXACT["gu"] = [[fn(e, (x, y)) for e in row] for row in gu]
        _EXACT["f"] = [fn(e, (x, y, p)) for e in f]
    return _EXACT


def _points(mesh, qp):
    J = chk.cell_geometry(mesh)[0]
    xq = mesh.x[mesh.cell_nodes[:, 0], :2][:, None, :] + np.einsum("cij,qj->cqi", J, qp)
    return xq[..., 0], xq[..., 1]


def elasticity_problem(n, k, pi_1):
    """The P_k Galerkin solution on create_unit_square(n, shuffle_seed=3, perturb=0.15) and what the equilibration and the
    estimate need: dict(mesh, ft [2, nfacets], cd, b, u [ndofs, 2], G [2, .] rows of -sigma(u_h) at the DG_{k-1} nodes,
    fh [2, .] = Pi_{k-1} f, osc2 [ncells] = sum_r || f_r - Pi f_r ||^2_T, h, err)."""
    import scipy.sparse.linalg as spla
    import elasticity_cases as ec
    from dolfinx_eqlb_amd.elmtlib.lagrange import Lagrange
    from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
    ex = elasticity_exact()
    mesh = create_unit_square(n, shuffle_seed=3, perturb=0.15)
    A = ec.assemble(mesh, k, pi_1)[0]
    cd, ndofs = gk.dofmap(mesh, k)
    el = Lagrange(k)
    J, detJ, K = chk.cell_geometry(mesh)
    qp, qw = make_quadrature_triangle(2 * k + 6)
    tab = el.tabulate(qp, 1)
    w = qw[None, :] * np.abs(detJ)[:, None]
    xq, yq = _points(mesh, qp)
    b = np.zeros(2 * ndofs)
    for r in range(2):
        np.add.at(b, (2 * cd + r).ravel(), np.einsum("cq,cq,qi->ci", w, ex["f"][r](xq, yq, pi_1), tab[0]).ravel())
    bf = mesh.boundary_facets()
    fixed = np.zeros(ndofs, dtype=bool)
    fixed[mesh.facet_nodes[bf].ravel()] = True
    for j in range(k - 1):
        fixed[mesh.nnodes + bf * (k - 1) + j] = True
    free = np.nonzero(~np.repeat(fixed, 2))[0]
    u = np.zeros(2 * ndofs)
    u[free] = spla.spsolve(A[free][:, free].tocsc(), b[free])
    u = u.reshape(ndofs, 2)
    fh, osc2 = [], 0.0
    for r in range(2):
        fr, o2, h = gk.project_rhs(mesh, k, lambda a, c, r=r: ex["f"][r](a, c, pi_1))
        fh.append(fr)
        osc2 = osc2 + o2
    ft = np.repeat(facet_types(mesh, None), 2, axis=0)
    return dict(mesh=mesh, ft=ft, cd=cd, b=b, u=u, G=elasticity_stress_rows(mesh, k, u, cd, pi_1), fh=np.stack(fh),
                osc2=osc2, h=h, err=elasticity_error(mesh, k, u, cd, pi_1), fixed=fixed)


def elasticity_stress_rows(mesh, k, u, cd, pi_1):
    """rows of -(2 eps(u_h) + pi_1 div(u_h) I) at the DG_{k-1} nodes: [2, ncells*nd*2] (exact: it lies in P_{k-1})"""
    from dolfinx_eqlb_amd.elmtlib.lagrange import Lagrange
    K = chk.cell_geometry(mesh)[2]
    nodes = np.array([[float(a), float(b)] for a, b in Lagrange(k - 1).nodes])
    tab = Lagrange(k).tabulate(nodes, 1)
    dphi = np.stack([tab[1], tab[2]], axis=2)                                  # [node, i, X]
    gu = np.einsum("cXd,niX,cir->cnrd", K, dphi, u[cd])                        # d_d u_r
    sig = gu + np.swapaxes(gu, 2, 3)
    div = gu[..., 0, 0] + gu[..., 1, 1]
    sig[..., 0, 0] += pi_1 * div
    sig[..., 1, 1] += pi_1 * div
    return np.ascontiguousarray(-np.moveaxis(sig, 2, 0).reshape(2, -1))


def elasticity_error(mesh, k, u, cd, pi_1):
    """sqrt(int 2 eps(e) : eps(e) + pi_1 (div e)^2), e = u - u_h, by quadrature of degree 2 k + 6"""
    from dolfinx_eqlb_amd.elmtlib.lagrange import Lagrange
    from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
    ex = elasticity_exact()
    J, detJ, K = chk.cell_geometry(mesh)
    qp, qw = make_quadrature_triangle(2 * k + 6)
    tab = Lagrange(k).tabulate(qp, 1)
    dphi = np.stack([tab[1], tab[2]], axis=2)
    guh = np.einsum("cXd,qiX,cir->cqrd", K, dphi, u[cd])
    xq, yq = _points(mesh, qp)
    ge = np.stack([np.stack([ex["gu"][r][d](xq, yq) for d in range(2)], axis=-1) for r in range(2)], axis=-2) - guh
    eps = 0.5 * (ge + np.swapaxes(ge, 2, 3))
    dens = 2.0 * np.einsum("cqrd,cqrd->cq", eps, eps) + pi_1 * (ge[..., 0, 0] + ge[..., 1, 1]) ** 2
    return float(np.sqrt(np.sum(qw[None, :] * np.abs(detJ)[:, None] * dens)))


def elasticity_estimate(energy, wsym, osc):
    """eta as the reference's estimate() sums it with guarantied_upper_bound=True (demo_error_estimation.py:134-148)"""
    return float(np.sqrt(np.sum(energy) + np.sum((np.sqrt(wsym) + np.sqrt(osc)) ** 2)))


def elasticity_host_terms(oracle_mod, P, k, pi_1):
    """(energy, wsym, osc per cell, C_K per cell) of the host chain: oracle with weak symmetry and Korn constants, the
    numpy statements of check_eqlb_conditions"""
    mesh = P["mesh"]
    x = oracle_mod.se_reconstruct(mesh, k, P["ft"], P["G"], P["fh"], stress=True)
    for r in range(2):
        res, nrm = chk.divergence_residual(mesh, k, x[r], P["G"][r], P["fh"][r])
        assert res < 1e-9 * nrm and chk.check_jump_condition(mesh, k, x[r], P["G"][r], atol=1e-9 * np.abs(P["G"]).max())
    # The weak symmetry condition holds to rounding at k >= 3 only.  At k = 2 the patch problems see Pi_1 f where the
    # Galerkin solution saw f, and hat_a times a rotation is a P_2 field that Pi_1 f does not reproduce: the oracle leaves
    # an asymmetry of the order of the oscillation there (1.4e-3 at n = 4, 3.2e-5 at n = 8, scale 29); the estimate
    # measures it in its wsym term.
    if k >= 3:
        assert chk.weak_symmetry_residual(mesh, k, x)[0] < 1e-10 * np.abs(P["G"]).max()
    korn = np.sqrt(oracle_mod.se_korn(mesh, P["ft"]))
    energy, wsym = chk.stress_estimator_terms(mesh, k, x, korn, pi_1)
    return energy, wsym, korn ** 2 * (P["h"] / np.pi) ** 2 * P["osc2"], korn


@pytest.mark.parametrize("pi_1", [1.0, 100.0])
@pytest.mark.parametrize("k", [2, 3])
def test_elasticity_guaranteed_upper_bound(oracle_mod, k, pi_1):
    """eta^2 = sum energy + sum (sqrt(wsym) + sqrt(osc))^2 bounds the energy error of the P_k solution from above on
    every level, and the error converges with order k.  The effectivity is large because of the Korn constants
    (C_K = 11.5 ... 25.8 on these meshes), so no sharpness is asserted.  Measured (n = 4 / 8 / 16):
      k = 2, pi_1 = 1    eta / e 19.68 / 12.59 / 9.72,   error rates 1.954, 1.980, sqrt(sum energy) / e 1.22 ... 1.23,
                         sqrt(sum wsym) / e 10.2 / 8.5 / 7.8, sqrt(sum osc) / e 9.7 / 4.4 / 2.1
      k = 3, pi_1 = 1    eta / e 20.90 / 14.48 / 11.15,  error rates 2.982, 2.994, sqrt(sum energy) / e 1.11 ... 1.13
      k = 2, pi_1 = 100  eta / e 155.5 / 98.8 / 70.8,    error rates 2.003, 1.967, sqrt(sum energy) / e 7.98 ... 8.18
      k = 3, pi_1 = 100  eta / e 161.8 / 93.1 / 67.6,    error rates 2.922, 3.031, sqrt(sum energy) / e 7.61 ... 7.68"""
    eff, errs = [], []
    for n in (4, 8, 16):
        P = elasticity_problem(n, k, pi_1)
        energy, wsym, osc, korn = elasticity_host_terms(oracle_mod, P, k, pi_1)
        eta = elasticity_estimate(energy, wsym, osc)
        eff.append(eta / P["err"])
        errs.append(P["err"])
        print(f"k={k} pi_1={pi_1:g} n={n}: e = {P['err']:.6e}, eta / e = {eff[-1]:.3f}, sqrt(sum energy) / e = "
              f"{np.sqrt(energy.sum()) / P['err']:.4f}, sqrt(sum wsym) / e = {np.sqrt(wsym.sum()) / P['err']:.4f}, "
              f"sqrt(sum osc) / e = {np.sqrt(osc.sum()) / P['err']:.4f}, C_K in [{korn.min():.2f}, {korn.max():.2f}]")
        assert eta / P["err"] >= 1.0 - 1e-10, eff
    rates = [float(np.log2(errs[i] / errs[i + 1])) for i in range(2)]
    print(f"k={k} pi_1={pi_1:g}: error rates {rates[0]:.3f}, {rates[1]:.3f}")
    assert rates[1] > k - 0.2, rates


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 3])
def test_gpu_elasticity_pipeline_bound(oracle_mod, k):
    """The same chain on the device: PrimalElasticity solve -> primal_stress_dg -> project_dg -> stress equilibration
    with Korn constants -> estimate_stress -> oscillation with korn -> indicator_total(pair_last_two=True).  The bound
    holds, and each of the three totals agrees with the host chain (sparse direct solve, oracle, numpy statements) within
    1e-9, the margin of test_gpu_pipeline_bound."""
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
    n, pi_1 = 8, 1.0
    P = elasticity_problem(n, k, pi_1)
    mesh, ex = P["mesh"], elasticity_exact()
    host = elasticity_host_terms(oracle_mod, P, k, pi_1)
    dm = cpp.DeviceMesh(mesh)
    solver = cpp.PrimalElasticity(dm, k, pi_1)
    assert np.array_equal(dm.lagrange_dofmap(k)[0], P["cd"])      # the numbering the host load b is written in
    bf = mesh.boundary_facets().astype(np.int32)
    solver.set_dirichlet(bf, bf)
    u, info = solver.solve(P["b"], np.zeros(2 * solver.ndofs), rtol=1e-13, maxit=20000)
    assert info["converged"], info
    G = cpp.primal_stress_dg(dm, k, k - 1, P["cd"].astype(np.int32), u, pi_1)
    qp, qw = make_quadrature_triangle(2 * k + 6)
    xq, yq = _points(mesh, qp)
    fv = np.stack([ex["f"][r](xq, yq, pi_1) for r in range(2)])
    fh = cpp.project_dg(dm, k - 1, qp, qw, fv[:, :, :, None])
    eq = cpp.SemiExplicitEquilibrator(dm, k, 2, reconstruct_stress=True, estimate_korn=True)
    eq.set_boundary(P["ft"])
    x, ck2 = eq.equilibrate_host_with_kornconst(G, fh)
    korn = np.sqrt(ck2)
    energy, wsym, asym = cpp.estimate_stress(dm, k, x, korn, pi_1)
    if k >= 3:                                               # k = 2: see elasticity_host_terms
        assert np.abs(asym).max() < 1e-10 * np.abs(G).max()
    osc = cpp.oscillation(dm, k, x, G, qp, qw, fv, korn).sum(axis=0)
    eta2, totals = cpp.indicator_total([energy, wsym, osc], pair_last_two=True)
    eta = float(np.sqrt(totals[3]))
    print(f"k={k}: eta_device / e = {eta / P['err']:.4f}; totals device {totals[:3]}, host {[float(t.sum()) for t in host[:3]]}")
    assert eta / P["err"] >= 1.0 - 1e-10
    for name, dev, ref in zip(("energy", "wsym", "osc"), totals[:3], host[:3]):
        assert abs(dev - ref.sum()) <= 1e-9 * ref.sum(), (name, dev, ref.sum())
