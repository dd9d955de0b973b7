"""Host-memory calls on a caller's (non-blocking) stream.  A host-memory call is the device-memory call staged and
synchronous: inputs go up, the kernels run and the outputs come back on the CALLER's stream, and the call returns when
that stream has finished.  Every entry point below is called twice with the same host arrays: on a torch stream that
is still busy with a spin kernel when the call arrives (a copy back that is not ordered behind the call's own kernels
on that stream returns what the staging buffer held before they ran), and on stream 0.  The two results have to be
equal bit for bit, and every output element has to be written (outputs start as NaN or as a sentinel no call
produces).  The failure looked for is one of ordering, not of arithmetic: 64 cells, k = p = 2, two right-hand sides,
random data."""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, P, R = 2, 2, 2
NRT, ND, NDP = K * (K + 2), K * (K + 1) // 2, (P + 1) * (P + 2) // 2
SENTINEL = -7777  # (no id, offset or count is negative but the -1 of "no such facet")


def _nan(*shape):
    return np.full(shape, np.nan)


def _ids(*shape, dtype=np.int32):
    return np.full(shape, 255 if dtype == np.uint8 else SENTINEL, dtype=dtype)


class Ctx:
    """Mesh, handles and input data, made once; the calls only read them."""

    def __init__(self):
        from dolfinx_eqlb_amd import cpp
        from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
        from dolfinx_eqlb_amd.mesh import create_unit_square
        from synthetic import facet_types
        rng = np.random.default_rng(20261019)
        self.cpp = cpp
        self.mesh = m = create_unit_square(4, shuffle_seed=2, perturb=0.15)
        assert m.ncells == 64
        self.dm = cpp.DeviceMesh(m)
        nc = m.ncells
        self.x = rng.standard_normal((R, nc * NRT))
        self.G = rng.standard_normal((R, nc * ND * 2))
        self.f = rng.standard_normal((R, nc * ND))
        self.korn = 1.0 + rng.random(nc)
        self.bv = rng.standard_normal((R, nc * NRT))
        self.qp, self.qw = [np.ascontiguousarray(a, dtype=np.float64) for a in make_quadrature_triangle(3)]
        self.nq = self.qw.size
        self.qv = rng.standard_normal((R, nc, self.nq, 1))
        self.fv = rng.standard_normal((R, nc, self.nq))
        self.terms = [rng.random(nc) for _ in range(3)]
        self.eta2 = rng.random(nc)
        gs, gw = np.polynomial.legendre.leggauss(3)
        self.s, self.w = 0.5 * (gs + 1.0), 0.5 * gw
        self.bf = np.ascontiguousarray(m.boundary_facets(), dtype=np.int32)
        ft = facet_types(m, lambda xm: xm[:, 0] < 0.3, nrhs=R)
        self.flux_facets = np.ascontiguousarray(np.nonzero(ft[0] == 2)[0], dtype=np.int32)
        assert self.flux_facets.size > 0
        self.bc_values = rng.standard_normal((self.flux_facets.size, self.s.size))
        self.bf_values = rng.standard_normal((self.bf.size, self.s.size))
        self.se = cpp.SemiExplicitEquilibrator(self.dm, K, R)
        self.se.set_boundary(ft)
        self.stress = cpp.SemiExplicitEquilibrator(self.dm, K, 2, reconstruct_stress=True)
        self.stress.set_boundary(facet_types(m, None, nrhs=2))
        self.cd, self.ndofs = self.dm.lagrange_dofmap(P)
        self.u = rng.standard_normal((R, self.ndofs))
        self.u_blocked = rng.standard_normal((self.ndofs, 2))
        # a refinement of three cells: plan and refined mesh
        ids = np.array([0, 5, 17], dtype=np.int32)
        count = np.array([ids.size], dtype=np.int64)
        self.plan = self.dm.refine_raw(ids.ctypes.data, count.ctypes.data, ids.size, cpp.MEM_HOST, 0)
        self.nn2, self.nc2, self.nbis, _ = self.plan.counts()
        assert self.nbis > 0
        self.dm2 = self.plan.create_mesh()
        self.nf2 = self.dm2.counts()[2]
        self.cd2, self.ndofs2 = self.dm2.lagrange_dofmap(P)
        self.dg = rng.standard_normal((R, nc * ND * 2))

    def close(self):
        self.plan.close()
        for h in (self.se, self.stress, self.dm2, self.dm):
            h.close()


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


def _p(a):
    return a.ctypes.data


# ---- one function per entry point: (ctx, stream) -> the output arrays of a host-memory call --------------------------
def project_dg(c, st):
    out = _nan(R, c.mesh.ncells * ND)
    c.cpp._check(c.cpp.lib().eqlb_project_dg(c.dm._h, C.c_int32(K - 1), C.c_int32(1), C.c_int32(R), C.c_int32(c.nq),
                                             c.cpp._hp(c.qp), c.cpp._hp(c.qw), c.cpp._hp(c.qv), c.cpp._hp(out),
                                             C.c_int32(c.cpp.MEM_HOST), C.c_void_p(st)))
    return [out]


def se_estimate(c, st):
    div2, sig2, jump = _nan(R, c.mesh.ncells), _nan(R, c.mesh.ncells), _nan(R, c.mesh.nfacets)
    c.cpp.estimate_raw(c.dm, K, R, _p(c.x), _p(c.G), _p(c.f), _p(div2), _p(sig2), _p(jump), memspace=c.cpp.MEM_HOST,
                       stream=st)
    return [div2, sig2, jump]


def se_estimate_stress(c, st):
    energy, wsym, asym = _nan(c.mesh.ncells), _nan(c.mesh.ncells), _nan(c.mesh.nnodes)
    c.cpp._check(c.cpp.lib().eqlb_se_estimate_stress(c.dm._h, C.c_int32(K), c.cpp._hp(c.x), c.cpp._hp(c.korn),
                                                     C.c_double(1.5), c.cpp._hp(energy), c.cpp._hp(wsym),
                                                     c.cpp._hp(asym), C.c_int32(c.cpp.MEM_HOST), C.c_void_p(st)))
    return [energy, wsym, asym]


def oscillation(c, st):
    out = _nan(R, c.mesh.ncells)
    c.cpp.oscillation_raw(c.dm, K, R, _p(c.x), _p(c.G), c.qp, c.qw, _p(c.fv), _p(c.korn), _p(out),
                          memspace=c.cpp.MEM_HOST, stream=st)
    return [out]


def boundary_residual(c, st):
    out = _nan(R, c.bf.size)
    c.cpp.boundary_residual_raw(c.dm, K, K - 1, R, _p(c.x), _p(c.G), c.bf.size, _p(c.bf), _p(c.bv), _p(out),
                                c.cpp.MEM_HOST, st)
    return [out]


def indicator_total(c, st):
    eta2, totals = _nan(c.mesh.ncells), _nan(len(c.terms) + 1)
    c.cpp.indicator_total_raw(c.mesh.ncells, [_p(t) for t in c.terms], True, _p(eta2), _p(totals), c.cpp.MEM_HOST, st)
    return [eta2, totals]


def mark_doerfler(c, st):
    marked = _ids(c.mesh.ncells)
    nmarked, total = C.c_int64(0), C.c_double(np.nan)
    c.cpp.mark_doerfler_raw(c.mesh.ncells, _p(c.eta2), 0.5, _p(marked), C.addressof(nmarked), C.addressof(total),
                            c.cpp.MEM_HOST, st)
    n = int(nmarked.value)
    assert 1 <= n < c.mesh.ncells and (marked[n:] == SENTINEL).all()  # (only marked[0 .. nmarked) is written)
    return [marked[:n], np.array([n]), np.array([total.value])]


def primal_flux_dg(c, st):
    out = _nan(R, c.mesh.ncells * ND * 2)
    c.cpp.primal_flux_dg_raw(c.dm, P, K - 1, R, _p(c.cd), c.ndofs, _p(c.u), _p(c.korn), _p(out),
                             memspace=c.cpp.MEM_HOST, stream=st)
    return [out]


def primal_stress_dg(c, st):
    out = _nan(2, c.mesh.ncells * ND * 2)
    c.cpp.primal_stress_dg_raw(c.dm, P, K - 1, _p(c.cd), c.ndofs, _p(c.u_blocked), 1.5, _p(c.korn), _p(out),
                               memspace=c.cpp.MEM_HOST, stream=st)
    return [out]


def facet_points(c, st):
    xq = _nan(c.bf.size, c.s.size, 2)
    c.cpp.facet_points_raw(c.dm, c.bf.size, _p(c.bf), c.s, _p(xq), c.cpp.MEM_HOST, st)
    return [xq]


def flux_bc_dofs(c, st):
    dofs = _nan(c.bf.size, K)
    c.cpp.flux_bc_dofs_raw(c.dm, K, c.bf.size, _p(c.bf), c.s, c.w, _p(c.bf_values), False, _p(dofs), c.cpp.MEM_HOST,
                           st)
    return [dofs]


def update_flux_bc(c, st):
    table = _nan(R, c.mesh.ncells * NRT)
    c.se.update_flux_bc_raw(0, c.flux_facets.size, _p(c.flux_facets), _p(c.bc_values), c.s, c.w, False, None,
                            c.cpp.MEM_HOST, st)
    c.se.get_boundary_values_raw(_p(table), c.cpp.MEM_HOST, st)
    assert np.count_nonzero(table) > 0
    return [table]


def se_kornconst(c, st):
    korn = np.zeros(c.mesh.ncells)  # (the constants are added to it)
    c.cpp._check(c.cpp.lib().eqlb_se_kornconst(c.stress._h, c.cpp._hp(korn), C.c_int32(c.cpp.MEM_HOST),
                                               C.c_void_p(st)))
    assert np.count_nonzero(korn) > 0
    return [korn]


def se_equilibrate(c, st):
    x = np.zeros((R, c.mesh.ncells * NRT))  # (the flux is added to it)
    c.cpp._check(c.cpp.lib().eqlb_se_equilibrate(c.se._h, c.cpp._hp(c.G), c.cpp._hp(c.f), c.cpp._hp(x),
                                                 C.c_int32(c.cpp.MEM_HOST), C.c_void_p(st)))
    assert all(np.count_nonzero(row) > 0 for row in x)
    return [x]


def refine_write(c, st):
    x2, cn2 = _nan(c.nn2, 3), _ids(c.nc2, 3)
    pc, npf = _ids(c.nc2), _ids(c.nbis)
    c.plan.write_raw(_p(x2), _p(cn2), _p(pc), _p(npf), c.cpp.MEM_HOST, st)
    return [x2, cn2, pc, npf]


def refine_parent_facets(c, st):
    pf = _ids(c.nf2)
    c.plan.parent_facets_raw(c.dm2, _p(pf), c.cpp.MEM_HOST, st)
    return [pf]


def refine_prolong_lagrange(c, st):
    u2 = _nan(R, c.ndofs2)  # (every DOF of the conforming space is named by cell_dofs2, so every entry is written)
    c.plan.prolong_lagrange_raw(c.dm2, P, 1, R, _p(c.cd), c.ndofs, _p(c.u), _p(c.cd2), c.ndofs2, _p(u2),
                                c.cpp.MEM_HOST, st)
    return [u2]


def refine_prolong_dg(c, st):
    out = _nan(R, c.nc2 * ND * 2)
    c.plan.prolong_dg_raw(c.dm2, K - 1, 2, R, _p(c.dg), _p(out), c.cpp.MEM_HOST, st)
    return [out]


def mesh_lagrange_dofmap(c, st):
    cd = _ids(c.mesh.ncells, NDP)
    assert c.dm.lagrange_dofmap_raw(P, _p(cd), c.cpp.MEM_HOST, st) == c.ndofs
    return [cd]


def mesh_export(c, st):
    m = c.mesh
    t = {"cell_facets": _ids(m.ncells, 3), "facet_nodes": _ids(m.nfacets, 2),
         "facet_cells_offsets": _ids(m.nfacets + 1), "facet_cells": _ids(len(m.facet_cells)),
         "node_cells_offsets": _ids(m.nnodes + 1), "node_cells": _ids(len(m.node_cells)),
         "node_facets_offsets": _ids(m.nnodes + 1), "node_facets": _ids(len(m.node_facets)),
         "facet_perm": _ids(m.ncells, 3, dtype=np.uint8)}
    c.dm.export_raw(**{name: _p(a) for name, a in t.items()}, memspace=c.cpp.MEM_HOST, stream=st)
    return list(t.values())


def mesh_boundary_facets(c, st):
    out = _ids(c.mesh.nfacets)
    status, n = c.dm.boundary_facets_raw(_p(out), out.size, c.cpp.MEM_HOST, st)
    assert status == 0 and n == c.bf.size
    return [out[:n]]


def mesh_find_facets(c, st):
    pairs = np.ascontiguousarray(c.mesh.facet_nodes, dtype=np.int32)
    out = _ids(pairs.shape[0])
    c.dm.find_facets_raw(pairs.shape[0], _p(pairs), _p(out), c.cpp.MEM_HOST, st)
    return [out]


CALLS = [project_dg, se_estimate, se_estimate_stress, oscillation, boundary_residual, indicator_total, mark_doerfler,
         primal_flux_dg, primal_stress_dg, facet_points, flux_bc_dofs, update_flux_bc, se_kornconst, se_equilibrate,
         refine_write, refine_parent_facets, refine_prolong_lagrange, refine_prolong_dg, mesh_lagrange_dofmap,
         mesh_export, mesh_boundary_facets, mesh_find_facets]


@pytest.mark.parametrize("call", CALLS, ids=[f.__name__ for f in CALLS])
def test_host_call_on_a_busy_user_stream(ctx, call):
    import torch
    s = torch.cuda.Stream(device=torch.device("cuda:0"))
    with torch.cuda.stream(s):
        torch.cuda._sleep(40_000_000)  # ~ 15-20 ms: the call's own work is queued behind it
    busy = call(ctx, s.cuda_stream)
    assert s.query()  # the call has waited for the caller's stream
    plain = call(ctx, 0)
    assert len(busy) == len(plain)
    for i, (a, b) in enumerate(zip(busy, plain)):
        if a.dtype.kind == "f":
            assert np.isfinite(a).all() and np.isfinite(b).all(), (call.__name__, i)
        else:
            unwritten = 255 if a.dtype == np.uint8 else SENTINEL
            assert (a != unwritten).all() and (b != unwritten).all(), (call.__name__, i)
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (call.__name__, i)
