"""Acceptance predicates of an equilibrated flux, restated on flat arrays.

Mirrors python/dolfinx_eqlb/eqlb/check_eqlb_conditions.py of the reference (which
needs DOLFINx Functions): divergence condition (:183-291), jump / H(div)-conformity
condition (:294-473), flux boundary condition (:90-179) and the reversed-edge
detector (:19-86).  Inputs are the arrays the C ABI works on:

  sigma_eq [ncells*k(k+2)]  corrector in the discontinuous hierarchic RT_k space
  flux_dg  [ncells*nd*2]    projected flux G (DG_{k-1}^2, components interleaved)
  rhs_dg   [ncells*nd]      projected right-hand side

The reconstructed flux is sigma_eq + G (FluxEqlbSE.get_reconstructed_fluxes).
"""

import numpy as np

from ..elmtlib import e_raviart_thomas as ert
from ..elmtlib.lagrange import Lagrange
from ..elmtlib.quadrature import make_quadrature_interval, make_quadrature_triangle


def cell_geometry(mesh):
    """J[c] = dx/dX (2x2), detJ[c], K[c] = J^-1 of the affine cell maps."""
    x = mesh.x[:, :2]
    cn = mesh.cell_nodes
    x0, x1, x2 = x[cn[:, 0]], x[cn[:, 1]], x[cn[:, 2]]
    J = np.stack([x1 - x0, x2 - x0], axis=2)  # J[c, i, j] = dx_i/dX_j
    detJ = J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0]
    K = np.empty_like(J)
    K[:, 0, 0] = J[:, 1, 1] / detJ
    K[:, 0, 1] = -J[:, 0, 1] / detJ
    K[:, 1, 0] = -J[:, 1, 0] / detJ
    K[:, 1, 1] = J[:, 0, 0] / detJ
    return J, detJ, K


def mesh_has_reversed_edges(mesh) -> bool:
    """True if some interior facet is traversed in opposite directions by its two cells
    (check_eqlb_conditions.py:19-86)."""
    off = mesh.facet_cells_offsets
    interior = np.nonzero(np.diff(off) == 2)[0]
    c0 = mesh.facet_cells[off[interior]]
    c1 = mesh.facet_cells[off[interior] + 1]
    l0 = np.argmax(mesh.cell_facets[c0] == interior[:, None], axis=1)
    l1 = np.argmax(mesh.cell_facets[c1] == interior[:, None], axis=1)
    return bool(np.any(mesh.facet_perm[c0, l0] != mesh.facet_perm[c1, l1]))


def _eval_flux(mesh, k, degree_dg, sigma_eq, flux_dg, ref_points, geom):
    """(sigma_eq + G) at reference points of every cell: [ncells, npts, 2]."""
    J, detJ, K = geom
    rt = ert.HierarchicRT(k)
    dg = Lagrange(degree_dg)
    phi = rt.tabulate(ref_points)  # [q, i, 2]
    psi = dg.tabulate(ref_points)[0]  # [q, j]
    c = sigma_eq.reshape(mesh.ncells, rt.ndofs)
    G = flux_dg.reshape(mesh.ncells, dg.ndofs, 2)
    ref = np.einsum("ci,qid->cqd", c, phi)
    val = np.einsum("cij,cqj->cqi", J, ref) / detJ[:, None, None]
    val += np.einsum("cjd,qj->cqd", G, psi)
    return val


def divergence_residual(mesh, k, sigma_eq, flux_dg, rhs_dg, degree_dg=None):
    """(|| div(sigma_eq + G) - f ||_L2, || f ||_L2): the 'L2 flux-divergence residual' of the
    headline metric (check_divergence_condition compares the same two fields pointwise)."""
    degree_dg = k - 1 if degree_dg is None else degree_dg
    J, detJ, K = cell_geometry(mesh)
    rt = ert.HierarchicRT(k)
    dg = Lagrange(degree_dg)
    qp, qw = make_quadrature_triangle(2 * k)
    divphi = rt.tabulate_div(qp)  # [q, i]
    tab = dg.tabulate(qp, 1)  # [3, q, j]
    c = sigma_eq.reshape(mesh.ncells, rt.ndofs)
    G = flux_dg.reshape(mesh.ncells, dg.ndofs, 2)
    f = rhs_dg.reshape(mesh.ncells, dg.ndofs)
    div_sig = np.einsum("ci,qi->cq", c, divphi) / detJ[:, None]
    # grad psi_j = K^T grad_ref psi_j
    dpsi = np.stack([tab[1], tab[2]], axis=2)  # [q, j, X]
    gpsi = np.einsum("cXd,qjX->cqjd", K, dpsi)
    div_G = np.einsum("cjd,cqjd->cq", G, gpsi)
    fq = np.einsum("cj,qj->cq", f, tab[0])
    res = div_sig + div_G - fq
    w = qw[None, :] * np.abs(detJ)[:, None]
    return float(np.sqrt(np.sum(w * res ** 2))), float(np.sqrt(np.sum(w * fq ** 2)))


def check_divergence_condition(mesh, k, sigma_eq, flux_dg, rhs_dg, degree_dg=None,
                               rtol=1e-5, atol=1e-8) -> bool:
    """Pointwise np.allclose of div(sigma_eq + G) and f (reference :280)."""
    degree_dg = k - 1 if degree_dg is None else degree_dg
    J, detJ, K = cell_geometry(mesh)
    rt = ert.HierarchicRT(k)
    dg = Lagrange(degree_dg)
    rng = np.random.default_rng(0)
    n_points = (k + 3) * (k + 4) // 2
    xs = np.sort(rng.random((2, n_points)), axis=0)
    pts = np.stack([xs[1] - xs[0], 1.0 - xs[1]], axis=1)  # barycentric weights of v1, v2
    divphi = rt.tabulate_div(pts)
    tab = dg.tabulate(pts, 1)
    c = sigma_eq.reshape(mesh.ncells, rt.ndofs)
    G = flux_dg.reshape(mesh.ncells, dg.ndofs, 2)
    f = rhs_dg.reshape(mesh.ncells, dg.ndofs)
    div_sig = np.einsum("ci,qi->cq", c, divphi) / detJ[:, None]
    dpsi = np.stack([tab[1], tab[2]], axis=2)
    gpsi = np.einsum("cXd,qjX->cqjd", K, dpsi)
    div_G = np.einsum("cjd,cqjd->cq", G, gpsi)
    fq = np.einsum("cj,qj->cq", f, tab[0])
    return bool(np.allclose(div_sig + div_G, fq, rtol=rtol, atol=atol))


def _facet_traces(mesh, k, degree_dg, sigma_eq, flux_dg, facets, side):
    """Outward normal flux density (w.r.t. ds of the unit parameter) of sigma_eq + G on the
    given facets, seen from cell `side` (0/1) of each facet, at matching physical points."""
    J, detJ, K = cell_geometry(mesh)
    s, w = make_quadrature_interval(2 * k)
    off = mesh.facet_cells_offsets
    cells = mesh.facet_cells[off[facets] + side]
    lf = np.argmax(mesh.cell_facets[cells] == facets[:, None], axis=1)
    perm = mesh.facet_perm[cells, lf]
    rt = ert.HierarchicRT(k)
    dg = Lagrange(degree_dg)
    c = sigma_eq.reshape(mesh.ncells, rt.ndofs)
    G = flux_dg.reshape(mesh.ncells, dg.ndofs, 2)
    out = np.zeros((facets.size, s.size))
    pf = np.where(np.array(ert.FACET_NORMAL_IS_OUTWARD), 1.0, -1.0)
    for f in range(3):
        for rev in (0, 1):
            sel = np.nonzero((lf == f) & (perm == rev))[0]
            if sel.size == 0:
                continue
            # parameter measured along the GLOBAL low->high direction of the facet
            sl = (1.0 - s) if rev else s
            pts = ert.facet_points(sl)[f]
            phi = rt.tabulate(pts)
            psi = dg.tabulate(pts)[0]
            cc = cells[sel]
            nref = np.array(ert.FACET_NORMALS[f], dtype=float)
            # sigma_eq: reference normal flux n_ref . phi_ref is the DOF density; outward
            # physical flux density = sign(detJ) * pf_f * that
            dens = np.einsum("ci,qi->cq", c[cc], phi @ nref) * (np.sign(detJ[cc]) * pf[f])[:, None]
            # G: pull back detJ K G, then the same functional density
            Gq = np.einsum("cjd,qj->cqd", G[cc], psi)
            pb = np.einsum("cXd,cqd->cqX", K[cc], Gq) * detJ[cc][:, None, None]
            dens += (pb @ nref) * (np.sign(detJ[cc]) * pf[f])[:, None]
            out[sel] = dens
    return out, w


def jump_residual(mesh, k, sigma_eq, flux_dg, degree_dg=None):
    """max over interior facets and points of |[(sigma_eq + G) . n]| (facet-length weighted
    flux density), cf. the per-facet variant check_eqlb_conditions.py:362-473."""
    degree_dg = k - 1 if degree_dg is None else degree_dg
    interior = np.nonzero(np.diff(mesh.facet_cells_offsets) == 2)[0]
    t0, _ = _facet_traces(mesh, k, degree_dg, sigma_eq, flux_dg, interior, 0)
    t1, _ = _facet_traces(mesh, k, degree_dg, sigma_eq, flux_dg, interior, 1)
    return float(np.max(np.abs(t0 + t1))) if interior.size else 0.0


def check_jump_condition(mesh, k, sigma_eq, flux_dg, degree_dg=None, atol=1e-10) -> bool:
    return jump_residual(mesh, k, sigma_eq, flux_dg, degree_dg) < atol


def boundary_flux_residual(mesh, k, sigma_eq, flux_dg, facets, degree_dg=None, boundary_values=None):
    """max |(sigma_eq + G) . n| on the given (flux-BC, homogeneous) boundary facets.
    boundary_values [ncells * k(k+2)] (the global boundary DOFs BoundaryData holds): max deviation of the
    facet DOFs of sigma_eq + G from them instead - check_boundary_conditions of the reference
    (check_eqlb_conditions.py:90-179) in the hierarchic basis, whose facet DOFs are the moments themselves."""
    degree_dg = k - 1 if degree_dg is None else degree_dg
    facets = np.asarray(facets, dtype=np.int64)
    if facets.size == 0:
        return 0.0
    if boundary_values is not None:
        J, detJ, K = cell_geometry(mesh)
        s, w = make_quadrature_interval(2 * k)
        cells = mesh.facet_cells[mesh.facet_cells_offsets[facets]]
        lf = np.argmax(mesh.cell_facets[cells] == facets[:, None], axis=1)
        nrt = k * (k + 2)
        dg = Lagrange(degree_dg)
        c = np.asarray(sigma_eq).reshape(mesh.ncells, nrt)
        G = np.asarray(flux_dg).reshape(mesh.ncells, dg.ndofs, 2)
        bv = np.asarray(boundary_values).reshape(mesh.ncells, nrt)
        worst = 0.0
        for f in range(3):
            sel = np.nonzero(lf == f)[0]
            if sel.size == 0:
                continue
            cc = cells[sel]
            psi = dg.tabulate(ert.facet_points(s)[f])[0]
            Gq = np.einsum("cjd,qj->cqd", G[cc], psi)
            pb = np.einsum("cXd,cqd->cqX", K[cc], Gq) * detJ[cc][:, None, None]
            dens = pb @ np.array(ert.FACET_NORMALS[f], dtype=float)
            for j in range(k):
                dof = c[cc, f * k + j] + dens @ (w * s ** j)
                worst = max(worst, float(np.max(np.abs(dof - bv[cc, f * k + j]))))
        return worst
    t0, _ = _facet_traces(mesh, k, degree_dg, sigma_eq, flux_dg, facets, 0)
    return float(np.max(np.abs(t0)))


def hdiv_seminorm_error(mesh, k, sigma_eq, flux_dg, rhs_exact, degree_dg=None):
    """|| div(sigma_eq + G) - f_exact ||_L2 for convergence-rate tests
    (python/test/unit/test_fluxeqlb_convrate.py:131-135)."""
    degree_dg = k - 1 if degree_dg is None else degree_dg
    J, detJ, K = cell_geometry(mesh)
    rt = ert.HierarchicRT(k)
    dg = Lagrange(degree_dg)
    qp, qw = make_quadrature_triangle(2 * k + 4)
    divphi = rt.tabulate_div(qp)
    tab = dg.tabulate(qp, 1)
    c = sigma_eq.reshape(mesh.ncells, rt.ndofs)
    G = flux_dg.reshape(mesh.ncells, dg.ndofs, 2)
    div_sig = np.einsum("ci,qi->cq", c, divphi) / detJ[:, None]
    dpsi = np.stack([tab[1], tab[2]], axis=2)
    gpsi = np.einsum("cXd,qjX->cqjd", K, dpsi)
    div_G = np.einsum("cjd,cqjd->cq", G, gpsi)
    x0 = mesh.x[mesh.cell_nodes[:, 0], :2]
    xq = x0[:, None, :] + np.einsum("cij,qj->cqi", J, qp)
    fq = rhs_exact(xq[..., 0], xq[..., 1])
    w = qw[None, :] * np.abs(detJ)[:, None]
    return float(np.sqrt(np.sum(w * (div_sig + div_G - fq) ** 2)))


def weak_symmetry_residual(mesh, k, sigma):
    """Assembled vector L_a = (sigma_01 - sigma_10, hat_a) over the P1 test space for a stress with
    the rows sigma [2, ncells*k(k+2)] (broken hierarchic RT_k); returns (max_a |L_a|, L).
    The linear form of check_weak_symmetry_condition, check_eqlb_conditions.py:476-521."""
    J, detJ, K = cell_geometry(mesh)
    rt = ert.HierarchicRT(k)
    qp, qw = make_quadrature_triangle(k + 2)
    phi = rt.tabulate(qp)
    hv = Lagrange(1).tabulate(qp)[0]
    c = np.asarray(sigma).reshape(2, mesh.ncells, rt.ndofs)
    # physical rows: J phi / detJ; only the components (row 0, y) and (row 1, x) are needed
    r0y = np.einsum("cj,ci,qij->cq", J[:, 1, :], c[0], phi) / detJ[:, None]
    r1x = np.einsum("cj,ci,qij->cq", J[:, 0, :], c[1], phi) / detJ[:, None]
    loc = np.einsum("cq,cq,qn->cn", qw[None] * np.abs(detJ)[:, None], r0y - r1x, hv)
    L = np.zeros(mesh.nnodes)
    np.add.at(L, mesh.cell_nodes.ravel(), loc.ravel())
    return float(np.abs(L).max()), L


def check_weak_symmetry_condition(mesh, k, sigma, rtol=1e-5, atol=1e-8) -> bool:
    """np.allclose(L, 0) as the reference (check_eqlb_conditions.py:517)."""
    return bool(np.allclose(weak_symmetry_residual(mesh, k, sigma)[1], 0.0, rtol=rtol, atol=atol))


def stress_estimator_terms(mesh, k, sigma, korn=None, pi_1=1.0, cell_pi1=None, mu=1.0, cell_mu=None):
    """Cell-wise terms of the stress estimator (demo/elasticity/demo_error_estimation.py:100-121), numpy
    statement with quadrature: (int dsig : A dsig, int (C_K (dsig_01 - dsig_10) / 2)^2) for the rows
    sigma [2, ncells*k(k+2)]; A tau = (tau - pi_1 / (2 + 2 pi_1) tr(tau) I) / 2.
    For sigma = mu_T (2 eps(u) + pi_T div(u) I) (eqlb_se_estimate_stress_mu): cell_pi1 [ncells] replaces the scalar pi_1,
    and both terms are divided by mu_T = cell_mu [ncells] where given, else the scalar mu - A_T = A(pi_T) / mu_T, and the
    Korn bound of the weak-symmetry term picks up 1 / mu_T since |||e|||^2_T >= 2 mu_T ||eps(e)||^2_T.  The defaults
    give the values without the keywords."""
    J, detJ, K = cell_geometry(mesh)
    rt = ert.HierarchicRT(k)
    qp, qw = make_quadrature_triangle(2 * k)
    phi = rt.tabulate(qp)
    c = np.asarray(sigma).reshape(2, mesh.ncells, rt.ndofs)
    val = np.einsum("cxa,rci,qia->rcqx", J, c, phi) / detJ[None, :, None, None]   # [row, cell, q, comp]
    w = qw[None] * np.abs(detJ)[:, None]
    fro = np.einsum("cq,rcqx,rcqx->c", w, val, val)
    tr = val[0, ..., 0] + val[1, ..., 1]
    asym = val[0, ..., 1] - val[1, ..., 0]
    ck = np.ones(mesh.ncells) if korn is None else np.asarray(korn)
    if cell_pi1 is not None:
        pi_1 = np.asarray(cell_pi1, dtype=np.float64).ravel()
    energy = 0.5 * (fro - pi_1 / (2.0 + 2.0 * pi_1) * np.einsum("cq,cq,cq->c", w, tr, tr))
    wsym = 0.25 * ck ** 2 * np.einsum("cq,cq,cq->c", w, asym, asym)
    if cell_mu is not None or mu != 1.0:
        m = np.asarray(cell_mu, dtype=np.float64).ravel() if cell_mu is not None else float(mu)
        if not np.all((m > 0.0) & np.isfinite(m)):
            raise ValueError("stress_estimator_terms: mu is zero, negative, NaN or infinite")
        energy, wsym = energy / m, wsym / m
    return energy, wsym


def det_sym2(d00, d01, d11):
    """d00 d11 - d01^2 within two units of the last place in the number type of the arrays (float64 or long double),
    however close the tensor is to singular: the two products are split exactly (Veltkamp / Dekker) and their
    residuals join the difference, as the fused multiply-adds of the estimator kernel do."""
    T = np.result_type(d00, d01, d11).type
    split = T(2.0 ** (27 if T is np.float64 else 32) + 1.0)

    def two_prod(a, b):
        p = a * b
        ah = split * a
        ah = ah - (ah - a)
        bh = split * b
        bh = bh - (bh - b)
        al, bl = a - ah, b - bh
        return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl

    a, b, c = np.asarray(d00, dtype=T), np.asarray(d01, dtype=T), np.asarray(d11, dtype=T)
    p1, e1 = two_prod(a, c)
    p2, e2 = two_prod(b, b)
    return (p1 - p2) + (e1 - e2)


_FLUX_NORM_TABLES = {}


def _flux_norm_tables(k, d):
    """Exact integrals over the reference triangle as nested lists of Fractions: S[a][b][i][j] = int phi_i^a phi_j^b of
    the hierarchic RT_k basis, R[a][i][e] = int phi_i^a chi_e and PP[e][g] = int chi_e chi_g with the DG_d nodal basis."""
    if (k, d) not in _FLUX_NORM_TABLES:
        from ..elmtlib import polynomials as P
        rt, dg = ert.HierarchicRT(k), Lagrange(d)
        comp = [[b[0] for b in rt.basis], [b[1] for b in rt.basis]]
        n, nd, I = rt.ndofs, dg.ndofs, P.integrate_triangle
        S = [[[[I(P.mul(comp[a][i], comp[b][j])) for j in range(n)] for i in range(n)] for b in range(2)]
             for a in range(2)]
        R = [[[I(P.mul(comp[a][i], dg.basis[e])) for e in range(nd)] for i in range(n)] for a in range(2)]
        PP = [[I(P.mul(dg.basis[e], dg.basis[g])) for g in range(nd)] for e in range(nd)]
        _FLUX_NORM_TABLES[(k, d)] = (S, R, PP)
    return _FLUX_NORM_TABLES[(k, d)]


def _rounded(nested, T):
    """Fractions rounded once to T: float for float64, head + tail for long double"""
    from fractions import Fraction
    a = np.array(nested, dtype=object)
    out = np.empty(a.shape, dtype=T)
    for idx in np.ndindex(a.shape):
        hi = float(a[idx])
        out[idx] = T(hi) if T is np.float64 else T(hi) + T(float(Fraction(a[idx]) - Fraction(hi)))
    return out


def weighted_flux_norm(mesh, k, sigma, flux_dg=None, degree_dg=None, coeff=None, cell_D=None, conforming=False,
                       dtype=np.float64, return_abs=False):
    """cell_sig2 [ncells] of eqlb_se_estimate_weighted / eqlb_ev_estimate_weighted, the numpy statement:
    int_T e^T W e with W_T = adj(D_T) / (kappa_T det D_T) = (kappa_T D_T)^-1, the flux error of -div(kappa D grad u) = f
    in its energy norm.  e = sigma (the corrector of the discontinuous SE flux; the total flux is sigma + G) or, with
    conforming=True, sigma - G (an EV flux in the broken layout), sigma [ncells*k(k+2)], G = flux_dg [ncells*nd*2] in
    DG_d^2, d = degree_dg (k - 1 if None).  coeff [ncells] is kappa (None: 1), cell_D [ncells, 3] = (d00, d01, d11)
    (None: the identity).  Quadrature-free, evaluated in `dtype` (np.float64 or np.longdouble) from the coordinates and
    exact reference integrals rounded once: with c the coefficients of a cell,
      sum_ab (J^T W J)_ab / |det J|  c^T S_ab c  - 2 sign(det J) sum c_i (J^T W G_e)_a R_aie  + |det J| sum G_e^T W G_g PP_eg
    (the last two terms with conforming=True only).  det D is formed by det_sym2.  return_abs: also the same expression
    on the absolute values of every factor and term, which bounds the rounding error of any evaluation order."""
    T = np.dtype(dtype).type
    d = k - 1 if degree_dg is None else int(degree_dg)
    S, R, PP = (_rounded(t, T) for t in _flux_norm_tables(k, d))
    nrt, nd, nc = k * (k + 2), (d + 1) * (d + 2) // 2, mesh.ncells
    x = mesh.x[:, :2].astype(T)
    cn = mesh.cell_nodes
    J = np.stack([x[cn[:, 1]] - x[cn[:, 0]], x[cn[:, 2]] - x[cn[:, 0]]], axis=2)       # J[c, x, a]
    det = J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0]
    kap = np.ones(nc, dtype=T) if coeff is None else np.asarray(coeff).astype(T).ravel()
    W = np.zeros((nc, 2, 2), dtype=T)
    if cell_D is None:
        W[:, 0, 0] = W[:, 1, 1] = T(1) / kap
    else:
        dd = np.asarray(cell_D).astype(T).reshape(nc, 3)
        iw = T(1) / (kap * det_sym2(dd[:, 0], dd[:, 1], dd[:, 2]))
        W[:, 0, 0], W[:, 0, 1], W[:, 1, 0], W[:, 1, 1] = dd[:, 2] * iw, -dd[:, 1] * iw, -dd[:, 1] * iw, dd[:, 0] * iw
    c = np.asarray(sigma).astype(T).reshape(nc, nrt)
    ad = np.abs(det)

    def quad(v, SS, M):
        u = np.einsum("abij,cj->cabi", SS, v)
        return np.einsum("cab,cab->c", M, np.einsum("ci,cabi->cab", v, u))

    M = np.einsum("cxa,cxy,cyb->cab", J, W, J) / ad[:, None, None]
    Ma = np.einsum("cxa,cxy,cyb->cab", np.abs(J), np.abs(W), np.abs(J)) / ad[:, None, None]
    val, A = quad(c, S, M), quad(np.abs(c), np.abs(S), Ma)
    if conforming:
        g = np.asarray(flux_dg).astype(T).reshape(nc, nd, 2)
        wg, wga = np.einsum("cxy,cey->cex", W, g), np.einsum("cxy,cey->cex", np.abs(W), np.abs(g))
        jg, jga = np.einsum("cxa,cex->cae", J, wg), np.einsum("cxa,cex->cae", np.abs(J), wga)
        sgn = np.where(det > 0, T(1), T(-1))
        sg = sgn * np.einsum("ci,cai->c", c, np.einsum("aie,cae->cai", R, jg))
        sga = np.einsum("ci,cai->c", np.abs(c), np.einsum("aie,cae->cai", np.abs(R), jga))
        gg = ad * np.einsum("cex,cex->c", wg, np.einsum("eg,cgx->cex", PP, g))
        gga = ad * np.einsum("cex,cex->c", wga, np.einsum("eg,cgx->cex", np.abs(PP), np.abs(g)))
        val, A = val - 2 * sg + gg, A + 2 * sga + gga
    return (val, A) if return_abs else val


def cell_diameter(mesh):
    """Longest edge per cell (dolfinx::mesh::h on triangles)."""
    x = mesh.x[mesh.cell_nodes, :2]
    e = np.stack([x[:, 1] - x[:, 0], x[:, 2] - x[:, 0], x[:, 2] - x[:, 1]], axis=1)
    return np.sqrt((e ** 2).sum(axis=2)).max(axis=1)


def oscillation_term(mesh, k, sigma, flux_dg, f, qdegree, korn=None, degree_dg=None):
    """C_K^2 (h_T/pi)^2 || f - div(sigma + G) ||^2_T per cell (demo/poisson/demo_error_estimation.py:96-98),
    numpy statement: f callable f(x, y), sigma [ncells*k(k+2)] broken hierarchic RT_k, flux_dg the DG_d^2
    part G of the total flux (d = degree_dg, k-1 if None) or None."""
    degree_dg = k - 1 if degree_dg is None else degree_dg
    J, detJ, K = cell_geometry(mesh)
    rt = ert.HierarchicRT(k)
    qp, qw = make_quadrature_triangle(qdegree)
    c = np.asarray(sigma).reshape(mesh.ncells, rt.ndofs)
    div = np.einsum("ci,qi->cq", c, rt.tabulate_div(qp)) / detJ[:, None]
    if flux_dg is not None:
        dg = Lagrange(degree_dg)
        gr = dg.tabulate(qp, 1)[1:]                               # [2, q, nd] reference derivatives
        G = np.asarray(flux_dg).reshape(mesh.ncells, dg.ndofs, 2)
        # d/dx_i = sum_a K[a, i] d/dX_a
        div = div + np.einsum("cai,aqd,cdi->cq", K, gr, G)
    x0 = mesh.x[mesh.cell_nodes[:, 0], :2]
    xq = x0[:, None, :] + np.einsum("cij,qj->cqi", J, qp)
    r = f(xq[..., 0], xq[..., 1]) - div
    ck = np.ones(mesh.ncells) if korn is None else np.asarray(korn)
    return ck ** 2 * (cell_diameter(mesh) / np.pi) ** 2 * np.abs(detJ) * np.einsum("q,cq->c", qw, r * r)
