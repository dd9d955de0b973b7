"""Estimators and acceptance predicates on the device with projected data of degree d, 0 <= d <= k-1, read as they
are (eqlb_se_estimate_dg, eqlb_ev_estimate_dg, eqlb_oscillation_dg) and the flux boundary condition
(eqlb_boundary_residual, check_eqlb_conditions.py:90-179 of the reference): against the numpy statements of
dolfinx_eqlb_amd/eqlb/check_eqlb_conditions.py at degree d, against the DG_{k-1} entry points on embed_dg(data), on
device-equilibrated fluxes, in both memory spaces.  Bounds as tests/test_gpu_estimate.py uses them for the same
quantities at d = k-1 (rtol 1e-11 / 1e-12, atol 1e-13 x max)."""

import numpy as np
import pytest

from cases import BCS, make_case
from dolfinx_eqlb_amd.elmtlib import e_raviart_thomas as ert
from dolfinx_eqlb_amd.elmtlib.lagrange import Lagrange
from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_interval, make_quadrature_triangle
from dolfinx_eqlb_amd.eqlb import check_eqlb_conditions as chk
from dolfinx_eqlb_amd.eqlb.conforming import broken_to_conforming
from dolfinx_eqlb_amd.lsolver import embed_dg
from dolfinx_eqlb_amd.mesh import create_unit_square
from synthetic import boundary_dofs_from_field, facet_types, make_compatible_data
from test_gpu_estimate import flux_norm2_cells

pytestmark = pytest.mark.gpu

PAIRS = [(k, d) for k in (1, 2, 3, 4) for d in range(k)]
IDS = [f"k{k}d{d}" for k, d in PAIRS]
QDEG = 8


@pytest.fixture(scope="module")
def cpp():
    from dolfinx_eqlb_amd import cpp as c
    assert c.device_count() >= 1, "GPU tests need a HIP device"
    return c


def nd_of(d):
    return (d + 1) * (d + 2) // 2


def f0(xx, yy):
    return np.sin(3.0 * xx) * np.exp(yy) + xx * yy


def f1(xx, yy):
    return np.cos(2.0 * xx + yy)


def f2(xx, yy):
    return 1.0 + xx * xx - 0.5 * yy


def random_case(k, d, nrhs=2, n=5, seed=4):
    """Arbitrary (non-equilibrated) coefficients on a perturbed mesh with shuffled local vertex orders
    (cells with det J < 0, facets seen in opposite directions)."""
    mesh = make_case(n, k, "dirichlet")[0]
    assert np.any(chk.cell_geometry(mesh)[1] < 0) and chk.mesh_has_reversed_edges(mesh)
    rng = np.random.default_rng(seed + 10 * k + d)
    x = rng.standard_normal((nrhs, mesh.ncells * k * (k + 2)))
    G = rng.standard_normal((nrhs, mesh.ncells * nd_of(d) * 2))
    f = rng.standard_normal((nrhs, mesh.ncells * nd_of(d)))
    return mesh, x, G, f


def embed(G, f, ncells, d, k):
    return (np.stack([embed_dg(g, ncells, d, k - 1, bs=2) for g in G]),
            np.stack([embed_dg(r, ncells, d, k - 1) for r in f]))


def fvalues(mesh, funcs):
    qp, qw = make_quadrature_triangle(QDEG)
    J = chk.cell_geometry(mesh)[0]
    xq = mesh.x[mesh.cell_nodes[:, 0], :2][:, None, :] + np.einsum("cij,qj->cqi", J, qp)
    return qp, qw, np.stack([fn(xq[..., 0], xq[..., 1]) for fn in funcs])


def ev_flux_error2(mesh, k, d, xb, G):
    """|| sigma - G ||^2_T per cell with G in DG_d (tests/test_estimator_bound.py: ev_flux_error2 at degree d)."""
    J, detJ, K = chk.cell_geometry(mesh)
    rt, dg = ert.HierarchicRT(k), Lagrange(d)
    qp, qw = make_quadrature_triangle(2 * k + 2)
    c = xb.reshape(mesh.ncells, rt.ndofs)
    sig = np.einsum("cdX,ci,qiX->cqd", J, c, rt.tabulate(qp)) / detJ[:, None, None]
    Gq = np.einsum("cjd,qj->cqd", G.reshape(mesh.ncells, dg.ndofs, 2), dg.tabulate(qp)[0])
    return np.einsum("q,cqd,cqd->c", qw, sig - Gq, sig - Gq) * np.abs(detJ)


def jump_moments(mesh, k, d, x, G):
    """max_j | int [(sigma_eq + G).n] s^j ds | per facet, s the facet parameter of the facet's first cell: the
    moments of the trace jump jump_residual takes the pointwise maximum of; 0 on boundary facets."""
    interior = np.nonzero(np.diff(mesh.facet_cells_offsets) == 2)[0]
    t0, w = chk._facet_traces(mesh, k, d, x, G, interior, 0)
    t1, _ = chk._facet_traces(mesh, k, d, x, G, interior, 1)
    s, _ = make_quadrature_interval(2 * k)
    c0 = mesh.facet_cells[mesh.facet_cells_offsets[interior]]
    l0 = np.argmax(mesh.cell_facets[c0] == interior[:, None], axis=1)
    sl = np.where(mesh.facet_perm[c0, l0][:, None] != 0, 1.0 - s[None, :], s[None, :])
    mom = np.stack([((t0 + t1) * w[None, :] * sl ** j).sum(axis=1) for j in range(k)], axis=1)
    out = np.zeros(mesh.nfacets)
    out[interior] = np.abs(mom).max(axis=1)
    return out


def close(a, b, rtol=1e-11):
    """The bounds of tests/test_gpu_estimate.py: rtol and 1e-13 x the largest value; the worst deviation is printed."""
    a, b = np.asarray(a), np.asarray(b)
    scale = np.abs(b).max()
    dev = np.abs(a - b).max()
    print(f"    max |a - b| = {dev:.3e}, max |b| = {scale:.3e}, ratio {dev / max(scale, 1e-300):.3e}")
    return np.allclose(a, b, rtol=rtol, atol=1e-13 * scale)


# ------------------------------------------------------------------------------- 1. the numpy statements at degree d
@pytest.mark.parametrize("k,d", PAIRS, ids=IDS)
def test_native_against_numpy_statements(cpp, k, d):
    mesh, x, G, f = random_case(k, d)
    dm = cpp.DeviceMesh(mesh)
    bnd = np.diff(mesh.facet_cells_offsets) == 1
    for ev in (False, True):
        div2, sig2, jump = cpp.estimate(dm, k, x, G, f, conforming_flux=ev, degree_dg=d)
        for r in range(x.shape[0]):
            Gt = np.zeros_like(G[r]) if ev else G[r]       # EV form: the total flux is sigma itself
            res, nrm = chk.divergence_residual(mesh, k, x[r], Gt, f[r], degree_dg=d)
            print(f"  ev={ev} r={r}: div {abs(np.sqrt(div2[r].sum()) - res) / res:.3e}")
            assert abs(np.sqrt(div2[r].sum()) - res) < 1e-11 * res
            ref = ev_flux_error2(mesh, k, d, x[r], G[r]) if ev else flux_norm2_cells(mesh, k, x[r])
            assert close(sig2[r], ref, rtol=1e-11 if ev else 1e-12)
            assert np.all(jump[r][bnd] == 0.0) and np.all(jump[r][~bnd] > 0.0)
            assert close(jump[r], jump_moments(mesh, k, d, x[r], Gt))
    # a conforming field has no jump: sigma_eq = 0, G = constant vector
    Gc = np.tile(np.array([0.3, -1.1]), mesh.ncells * nd_of(d))[None]
    _, _, j0 = cpp.estimate(dm, k, np.zeros_like(x[:1]), Gc, f[:1], degree_dg=d)
    assert j0.max() < 1e-13
    # outputs that are not wanted
    div_only = np.zeros((1, mesh.ncells))
    cpp.estimate_raw(dm, k, 1, x[:1].ctypes.data, G[:1].ctypes.data, f[:1].ctypes.data, div_only.ctypes.data, None,
                     None, degree_dg=d, memspace=cpp.MEM_HOST)
    assert np.array_equal(div_only[0], cpp.estimate(dm, k, x[:1], G[:1], f[:1], degree_dg=d)[0][0])
    # oscillation, with and without Korn constants, and for a conforming flux (no G)
    korn = 1.0 + np.random.default_rng(5).random(mesh.ncells)
    qp, qw, fv = fvalues(mesh, (f0, f1))
    out = cpp.oscillation(dm, k, x, G, qp, qw, fv, korn, degree_dg=d)
    for r, fr in enumerate((f0, f1)):
        assert close(out[r], chk.oscillation_term(mesh, k, x[r], G[r], fr, QDEG, korn, degree_dg=d))
    assert close(cpp.oscillation(dm, k, x[:1], None, qp, qw, fv[:1], degree_dg=d)[0],
                 chk.oscillation_term(mesh, k, x[0], None, f0, QDEG))


# ------------------------------------------------------------------------- 2. the DG_{k-1} entry points on embedded data
@pytest.mark.parametrize("k,d", PAIRS, ids=IDS)
def test_native_equals_embedded_route(cpp, k, d):
    """DG_d data and their embedding are the same polynomial; the two routes differ in the order of summation."""
    mesh, x, G, f = random_case(k, d, seed=9)
    Ge, fe = embed(G, f, mesh.ncells, d, k)
    dm = cpp.DeviceMesh(mesh)
    for ev in (False, True):
        nat = cpp.estimate(dm, k, x, G, f, conforming_flux=ev, degree_dg=d)
        emb = cpp.estimate(dm, k, x, Ge, fe, conforming_flux=ev)
        for name, a, b, rtol in zip(("div2", "sig2", "jump"), nat, emb, (1e-11, 1e-11 if ev else 1e-12, 1e-11)):
            print(f"  ev={ev} {name}:")
            assert close(a, b, rtol=rtol), name
    qp, qw, fv = fvalues(mesh, (f0, f1))
    assert close(cpp.oscillation(dm, k, x, G, qp, qw, fv, degree_dg=d), cpp.oscillation(dm, k, x, Ge, qp, qw, fv))


# ------------------------------------------------------------------------------------- 3. device-equilibrated fluxes
def galerkin_case(k, d, n):
    """Real Galerkin data for the pair: the P_p solution of tests/test_estimator_bound.py, p = min(d + 1, 3), whose
    flux and projected right-hand side live in DG_{p-1}; (4, 3) takes the P_3 data embedded into DG_3."""
    from test_estimator_bound import problem
    p = min(d + 1, 3)
    mesh, ft, G, fh, osc2, h, err = problem(n, p)
    if d > p - 1:
        G, fh = embed_dg(G, mesh.ncells, p - 1, d, bs=2), embed_dg(fh, mesh.ncells, p - 1, d)
    return mesh, ft, G, fh, err


@pytest.mark.parametrize("k,d", PAIRS, ids=IDS)
def test_estimate_on_device_equilibrated_flux(cpp, k, d):
    mesh, ft, G, fh, _ = galerkin_case(k, d, 8)
    dm = cpp.DeviceMesh(mesh)
    scale = np.abs(fh).max() ** 2 * np.abs(chk.cell_geometry(mesh)[1]).max()
    se = cpp.SemiExplicitEquilibrator(dm, k, 1, degree_dg=d)
    se.set_boundary(ft)
    x = se.equilibrate_host(G[None], fh[None])
    div2, sig2, jump = cpp.estimate(dm, k, x, G[None], fh[None], degree_dg=d)
    print(f"  SE: div2.max = {div2.max():.3e} (scale {scale:.3e}), jump.max = {jump.max():.3e}")
    assert div2.max() < 1e-20 * max(scale, 1.0) + 1e-22
    assert jump.max() < 1e-11
    ev = cpp.ConstrainedMinEquilibrator(dm, k, 1, degree_dg=d)
    ev.set_option("output", 1)
    ev.set_boundary(ft)
    xb = ev.equilibrate_host(G[None], fh[None])
    div2, sig2, jump = cpp.estimate(dm, k, xb, G[None], fh[None], conforming_flux=True, degree_dg=d)
    print(f"  EV: div2.max = {div2.max():.3e} (scale {scale:.3e}), jump.max = {jump.max():.3e}")
    assert div2.max() < 1e-20 * max(scale, 1.0) + 1e-22
    assert jump.max() < 1e-11


@pytest.mark.parametrize("k,d", [(2, 0), (3, 1)], ids=["k2d0", "k3d1"])
def test_prager_synge_bound_without_host_embedding(cpp, k, d):
    """P_{d+1} Galerkin solution -> RT_k equilibration with DG_d data -> eqlb_se_estimate_dg + eqlb_oscillation_dg:
    sum_T (|| sigma_eq ||_T + (h_T/pi) || f - div(sigma_eq + G) ||_T)^2 bounds the energy error from above
    (tests/test_estimator_bound.py).  Nothing is embedded on the host."""
    from test_estimator_bound import f_ex
    mesh, ft, G, fh, err = galerkin_case(k, d, 12)
    dm = cpp.DeviceMesh(mesh)
    se = cpp.SemiExplicitEquilibrator(dm, k, 1, degree_dg=d)
    se.set_boundary(ft)
    x = se.equilibrate_host(G[None], fh[None])
    div2, sig2, jump = cpp.estimate(dm, k, x, G[None], fh[None], degree_dg=d)
    assert np.sqrt(div2.sum()) < 1e-9 * np.sqrt(np.sum(fh ** 2)) and jump.max() < 1e-9
    qp, qw, fv = fvalues(mesh, (f_ex,))
    osc = cpp.oscillation(dm, k, x, G[None], qp, qw, fv, degree_dg=d)[0]
    eta = float(np.sqrt(np.sum(sig2[0] + osc + 2 * np.sqrt(sig2[0] * osc))))
    print(f"  effectivity index {eta / err:.4f}")
    assert eta / err >= 1.0 - 1e-10
    # the same estimate from the numpy statements
    ref = flux_norm2_cells(mesh, k, x[0])
    osc_ref = chk.oscillation_term(mesh, k, x[0], G, f_ex, QDEG, degree_dg=d)
    assert abs(eta - float(np.sqrt(np.sum(ref + osc_ref + 2 * np.sqrt(ref * osc_ref))))) <= 1e-9 * eta


# ------------------------------------------------------------------------------------- 4. the flux boundary condition
def w_lin(x, y):
    return 1.0 + 0.5 * x - 0.3 * y, -0.7 + 0.2 * x + 0.4 * y


def w_const(x, y):
    return 0 * x + 0.8, 0 * x - 0.6


def residual_per_facet(mesh, k, d, x, G, facets, bv):
    return np.array([chk.boundary_flux_residual(mesh, k, x, G, [fc], degree_dg=d, boundary_values=bv) for fc in facets])


def bc_case(k, d, inhomogeneous):
    """The set-up of tests/test_inhomogeneous_bc.py: a linear prescribed flux, a constant one at k = 1 (RT_1 cannot
    take hat_a times a linear flux on the corner patch of two flux-BC sides; the CPU oracle leaves 2.3e-4 on that
    facet as well)."""
    w_field = w_const if k == 1 else w_lin
    mesh = create_unit_square(6, shuffle_seed=8, perturb=0.25)
    ft = facet_types(mesh, BCS["neumann_lt"])
    G, f = make_compatible_data(mesh, k, ft, degree_dg=d, neumann_flux=w_field if inhomogeneous else None)
    bv = boundary_dofs_from_field(mesh, k, ft[0], w_field) if inhomogeneous else None
    bf = mesh.boundary_facets()
    return mesh, ft, G, f, bv, bf[ft[0][bf] == 2]


@pytest.mark.parametrize("inhomogeneous", [False, True], ids=["homogeneous", "inhomogeneous"])
@pytest.mark.parametrize("k,d", PAIRS, ids=IDS)
def test_boundary_residual(cpp, k, d, inhomogeneous):
    mesh, ft, G, f, bv, facets = bc_case(k, d, inhomogeneous)
    nrt = k * (k + 2)
    dm = cpp.DeviceMesh(mesh)
    bv2 = None if bv is None else bv[None]
    zero = np.zeros(mesh.ncells * nrt)
    cells = mesh.facet_cells[mesh.facet_cells_offsets[facets]]
    lf = np.argmax(mesh.cell_facets[cells] == facets[:, None], axis=1)
    fdofs = (cells * nrt + lf * k)[:, None] + np.arange(k)[None, :]          # facet DOFs of the listed facets
    # arbitrary coefficients: the numpy statement per facet
    rng = np.random.default_rng(3)
    xr = rng.standard_normal((1, mesh.ncells * nrt))
    got = cpp.boundary_residual(dm, k, xr, G[None], facets, bv2, degree_dg=d)
    assert got.shape == (1, facets.size)
    assert close(got[0], residual_per_facet(mesh, k, d, xr[0], G, facets, zero if bv is None else bv))
    assert close(cpp.boundary_residual(dm, k, xr, None, facets, bv2, degree_dg=d)[0],
                 residual_per_facet(mesh, k, d, xr[0], np.zeros_like(G), facets, zero if bv is None else bv))
    # SE form after equilibration: the facet DOFs of sigma_eq + G are the boundary DOFs
    se = cpp.SemiExplicitEquilibrator(dm, k, 1, degree_dg=d)
    se.set_boundary(ft, boundary_values=bv2)
    x = se.equilibrate_host(G[None], f[None])
    # the scale of the boundary DOFs: those of the data G and of the prescribed flux
    scale = max(residual_per_facet(mesh, k, d, zero, G, facets, zero).max(),
                0.0 if bv is None else np.abs(bv[fdofs]).max())
    res = cpp.boundary_residual(dm, k, x, G[None], facets, bv2, degree_dg=d)[0]
    ref = residual_per_facet(mesh, k, d, x[0], G, facets, zero if bv is None else bv)
    print(f"  SE: residual {res.max():.3e}, numpy {ref.max():.3e}, scale {scale:.3e}")
    assert res.max() < 1e-11 * scale and np.abs(res - ref).max() < 1e-11 * scale
    # a perturbed facet DOF is reported on its facet, and only there
    i, j, delta = facets.size // 2, k - 1, 0.37 * scale
    xp = x.copy()
    xp[0, fdofs[i, j]] += delta
    resp = cpp.boundary_residual(dm, k, xp, G[None], facets, bv2, degree_dg=d)[0]
    assert abs(resp[i] - delta) < 1e-11 * scale
    assert np.array_equal(np.delete(resp, i), np.delete(res, i)) and np.delete(resp, i).max() < 1e-11 * scale
    # EV form: a conforming flux in the broken layout is the total flux
    ev = cpp.ConstrainedMinEquilibrator(dm, k, 1, degree_dg=d)
    ev.set_option("output", 1)
    ev.set_boundary(ft, boundary_values=None if bv is None else broken_to_conforming(mesh, k, bv)[None])
    xb = ev.equilibrate_host(G[None], f[None])
    res = cpp.boundary_residual(dm, k, xb, None, facets, bv2, degree_dg=d)[0]
    ref = residual_per_facet(mesh, k, d, xb[0], np.zeros_like(G), facets, zero if bv is None else bv)
    print(f"  EV: residual {res.max():.3e}, numpy {ref.max():.3e}, scale {scale:.3e}")
    assert res.max() < 1e-11 * scale and np.abs(res - ref).max() < 1e-11 * scale
    assert cpp.boundary_residual(dm, k, xb, None, [], bv2, degree_dg=d).shape == (1, 0)


# ------------------------------------------------------------- 5. device memory, a caller's stream, several right-hand sides
@pytest.mark.parametrize("k,d", PAIRS, ids=IDS)
def test_device_memory_on_a_user_stream(cpp, k, d):
    """The calls of tests/test_gpu_streams.py for the estimator entry points: device-resident inputs that exist
    only late on a non-blocking stream (behind a spin kernel; NaN before and after), three right-hand sides with a
    field of degree d each, against the host-memory calls; two runs are bitwise equal."""
    import torch
    mesh, x, G, f = random_case(k, d, nrhs=3, n=12, seed=21)
    R = 3
    bv = np.random.default_rng(2).standard_normal(x.shape)
    facets = mesh.boundary_facets().astype(np.int32)
    qp, qw, fv = fvalues(mesh, (f0, f1, f2))
    dm = cpp.DeviceMesh(mesh)
    ref = cpp.estimate(dm, k, x, G, f, degree_dg=d)
    ref_ev = cpp.estimate(dm, k, x, G, f, conforming_flux=True, degree_dg=d)
    ref_osc = cpp.oscillation(dm, k, x, G, qp, qw, fv, degree_dg=d)
    ref_bnd = cpp.boundary_residual(dm, k, x, G, facets, bv, degree_dg=d)
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    src = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (x, G, f, fv, bv)]
    fl = torch.from_numpy(facets).to(dev)
    work = [torch.full_like(a, float("nan")) for a in src]
    outs = [torch.empty((R, n), dtype=torch.float64, device=dev)
            for n in (mesh.ncells, mesh.ncells, mesh.nfacets, mesh.ncells, mesh.ncells, mesh.nfacets, mesh.ncells,
                      facets.size)]
    torch.cuda.synchronize()
    runs = []
    for call in range(2):
        with torch.cuda.stream(s):
            torch.cuda._sleep(40_000_000)  # ~ 15-20 ms: the inputs below exist only after it
            for wk, a in zip(work, src):
                wk.copy_(a)
            for o in outs:
                o.fill_(float("nan"))
            xd, gd, fd, fvd, bvd = [wk.data_ptr() for wk in work]
            cpp.estimate_raw(dm, k, R, xd, gd, fd, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                             degree_dg=d, stream=s.cuda_stream)
            cpp.estimate_raw(dm, k, R, xd, gd, fd, outs[3].data_ptr(), outs[4].data_ptr(), outs[5].data_ptr(),
                             conforming_flux=True, degree_dg=d, stream=s.cuda_stream)
            cpp.oscillation_raw(dm, k, R, xd, gd, qp, qw, fvd, None, outs[6].data_ptr(), degree_dg=d,
                                stream=s.cuda_stream)
            cpp.boundary_residual_raw(dm, k, d, R, xd, gd, facets.size, fl.data_ptr(), bvd, outs[7].data_ptr(),
                                      stream=s.cuda_stream)
            got = [o.clone() for o in outs]
            for wk in work:
                wk.fill_(float("nan"))  # the inputs are gone right behind the calls
        s.synchronize()
        runs.append([g.cpu().numpy() for g in got])
    for a, b in zip(runs[0], runs[1]):
        assert np.isfinite(a).all() and np.array_equal(a, b)
    for a, b in zip(runs[0], list(ref) + list(ref_ev) + [ref_osc, ref_bnd]):
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
    # different fields per right-hand side give different results
    assert not np.allclose(runs[0][0][0], runs[0][0][1]) and not np.allclose(runs[0][7][1], runs[0][7][2])
    # a facet id outside the mesh: NaN for that entry in device memory, an error in host memory
    bad = torch.tensor([0, mesh.nfacets, -1], dtype=torch.int32, device=dev)
    o3 = torch.zeros((R, 3), dtype=torch.float64, device=dev)
    cpp.boundary_residual_raw(dm, k, d, R, src[0].data_ptr(), src[1].data_ptr(), 3, bad.data_ptr(), None,
                              o3.data_ptr())
    torch.cuda.synchronize()
    h3 = o3.cpu().numpy()
    assert np.isfinite(h3[:, 0]).all() and np.isnan(h3[:, 1:]).all()
    # a degree outside 0 ... k-1 never launches
    for badd in (-1, k):
        with pytest.raises(RuntimeError, match="Wrong polynomial degree"):
            cpp.estimate_raw(dm, k, R, src[0].data_ptr(), src[1].data_ptr(), src[2].data_ptr(), None, None, None,
                             degree_dg=badd)
        with pytest.raises(RuntimeError, match="Wrong polynomial degree"):
            cpp.boundary_residual_raw(dm, k, badd, R, src[0].data_ptr(), None, 3, bad.data_ptr(), None, o3.data_ptr())


# ----------------------------------------------------------------------------------------------------- 6. 1M triangles
def test_one_million_triangles_rt2_dg0(cpp):
    k, d = 2, 0
    mesh = create_unit_square(500, shuffle_seed=1234)
    rng = np.random.default_rng(0)
    x = rng.standard_normal((1, mesh.ncells * k * (k + 2)))
    G = rng.standard_normal((1, mesh.ncells * 2))
    f = rng.standard_normal((1, mesh.ncells))
    Ge, fe = embed(G, f, mesh.ncells, d, k)
    dm = cpp.DeviceMesh(mesh)
    for ev in (False, True):
        nat = cpp.estimate(dm, k, x, G, f, conforming_flux=ev, degree_dg=d)
        emb = cpp.estimate(dm, k, x, Ge, fe, conforming_flux=ev)
        for name, a, b, rtol in zip(("div2", "sig2", "jump"), nat, emb, (1e-11, 1e-11 if ev else 1e-12, 1e-11)):
            print(f"  ev={ev} {name}:")
            assert close(a, b, rtol=rtol), name
        assert all(np.array_equal(a, b)
                   for a, b in zip(nat, cpp.estimate(dm, k, x, G, f, conforming_flux=ev, degree_dg=d)))
