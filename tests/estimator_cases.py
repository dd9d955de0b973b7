"""Shared by tests/test_estimator_statements_host.py and tests/test_gpu_estimator_meshes.py: the meshes, the data, the
numpy statements and the bounds that hold the estimator kernels (k_estimate_cells, k_estimate_facets, k_boundary_residual,
k_oscillation_cells, k_estimate_stress_cells, k_gather_vertex_values, k_korn_patch, k_korn_cells) value by value.  No test
lives here.

Meshes.  Those of primal_mesh_cases.mesh_of (one and two cells, whole workgroups of 256, a vertex of 100 cells, a second
boundary loop, two components, a pinched vertex, an unstructured mesh, cells with det ~ 1e-14 far from the origin, det ~ 1e8,
aspect ratio 1000) and sq33: 4356 cells, 18 workgroups of the cell kernels, the last one partial.  check_table() asserts
what the table is there for.

Statements.  Statements(mesh, k, d, T) evaluates every output of the kernels in the number type T (np.float64 or
np.longdouble) from the coordinates, the coefficients and EXACT reference integrals: the tables below are integrals of the
exact rational basis polynomials of elmtlib (Fractions), rounded once to T.  No quadrature and no inverse matrix enters a
statement: the divergence residual is expanded in monomial coefficients and contracted with the monomial mass matrix,
where the kernels contract moments with its inverse (GMI).  Every statement returns (value, A), A the same expression on
the absolute values of every factor and term.

Bound.  |device - statement| <= c 2^-53 A per value, c = chain(...) below: the number of roundings along the longest chain
of the kernel plus that of the statement.  A dot product of n terms summed in any order is off by at most n roundings of
its abs-sum (n products, n - 1 additions; Higham, Accuracy and Stability, (3.5)), a rounded table entry, a difference of
coordinates, a product, a reciprocal count one each; a square doubles the count of its argument (|r| <= its abs-sum).
The counts are first order in 2^-53; c 2^-53 < 1e-12 everywhere, so the second order is below a thousandth of a unit.
Where the kernel goes through the moments and GMI (div2, oscillation), its own abs-sum |m|^T |GMI| |m| / |det J| is NOT
dominated by the statement's: GMI has entries of both signs up to 1e5 (k = 4).  There A is the sum of the two abs-sums,
each computation being bounded by its OWN one, as in primal_cases.chain_terms."""

import functools
import zlib
from fractions import Fraction
from math import comb

import numpy as np

import primal_mesh_cases as pm
from dolfinx_eqlb_amd.elmtlib import e_raviart_thomas as ert
from dolfinx_eqlb_amd.elmtlib import polynomials as P
from dolfinx_eqlb_amd.elmtlib.lagrange import Lagrange
from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle

U = 2.0 ** -53
MESHES = ["triangle", "right1", "wg256", "wg512", "delaunay", "disk100", "hole", "two_parts", "bowtie", "tiny_far", "huge",
          "aspect1000", "sq33"]
LOWDEG_MESHES_HOST = ["delaunay", "aspect1000"]
LOWDEG_MESHES_GPU = ["delaunay", "sq33", "aspect1000"]
RESHUFFLED = {"right1": 5, "delaunay": 5}       # name -> seed of the local vertex orders, see mesh_of
QDEG = 8
WG = 256


def nd_of(d):
    return (d + 1) * (d + 2) // 2


@functools.lru_cache(maxsize=None)
def mesh_of(name):
    if name == "sq33":
        from dolfinx_eqlb_amd.mesh import create_unit_square
        mesh = create_unit_square(33, shuffle_seed=11, perturb=0.2)
        assert (mesh.ncells, mesh.ncells // WG, mesh.ncells % WG) == (4356, 17, 4)
        return mesh
    mesh = pm.mesh_of(name)
    if name in RESHUFFLED:
        # the generators of these two orient every cell counter-clockwise: the same nodes and cells with a random local
        # vertex order per cell, so that the signs of det J and the facet reversal are met here as well
        from dolfinx_eqlb_amd.mesh import create_mesh
        rng = np.random.default_rng(RESHUFFLED[name])
        cn = np.stack([rng.permutation(row) for row in mesh.cell_nodes])
        shuffled = create_mesh(mesh.x[:, :2].copy(), cn)
        assert (shuffled.ncells, shuffled.nnodes, shuffled.nfacets) == (mesh.ncells, mesh.nnodes, mesh.nfacets)
        assert np.array_equal(np.sort(shuffled.cell_nodes, axis=1), np.sort(mesh.cell_nodes, axis=1))
        return shuffled
    return mesh


def geometry(mesh, T=np.float64):
    """(J[c, x, a] = dx_x / dX_a, det J, adj J with adj[c, a, x] = det J * (J^-1)[a, x]) from the coordinates in T"""
    x = mesh.x[:, :2].astype(T)
    cn = mesh.cell_nodes
    J = np.stack([x[cn[:, 1]] - x[cn[:, 0]], x[cn[:, 2]] - x[cn[:, 0]]], axis=2)
    det = J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0]
    adj = np.empty_like(J)
    adj[:, 0, 0], adj[:, 0, 1], adj[:, 1, 0], adj[:, 1, 1] = J[:, 1, 1], -J[:, 0, 1], -J[:, 1, 0], J[:, 0, 0]
    return J, det, adj


def has_reversed_facets(mesh):
    from dolfinx_eqlb_amd.eqlb.check_eqlb_conditions import mesh_has_reversed_edges
    return mesh_has_reversed_edges(mesh)


def check_table():
    """What the table is there for; a change of a generator cannot quietly empty a case."""
    meshes = {n: mesh_of(n) for n in MESHES}
    cells = [m.ncells for m in meshes.values()]
    assert any(c > WG and c % WG == 0 for c in cells) and any(c > WG and c % WG != 0 for c in cells)
    assert any(m.nfacets > WG and m.nfacets % WG != 0 for m in meshes.values())
    assert any(m.nnodes > WG and m.nnodes % WG != 0 for m in meshes.values())
    for n, m in meshes.items():
        if n != "triangle":
            assert np.any(geometry(m)[1] < 0) and has_reversed_facets(m), n
    assert pm.valence(meshes["disk100"]) == 100
    assert np.abs(geometry(meshes["tiny_far"])[1]).max() < 1e-13      # below the threshold a careless guard would take
    return meshes


# ---- exact reference tables ------------------------------------------------------------------------------------------
def _split(fr, T):
    """the Fraction rounded to T: float(fr) for float64, head + tail (106 bits) for long double"""
    hi = float(fr)
    return T(hi) if T is np.float64 else T(hi) + T(float(fr - Fraction(hi)))


def _arr(nested, T):
    a = np.array(nested, dtype=object)
    out = np.empty(a.shape, dtype=T)
    for idx in np.ndindex(a.shape):
        out[idx] = _split(Fraction(a[idx]), T)
    return out


def _coeffs(p, monos):
    assert all(e in monos for e in p), "polynomial outside the monomial space"
    return [p.get(e, Fraction(0)) for e in monos]


@functools.lru_cache(maxsize=None)
def exact_tables(k, d):
    """Integrals over the reference triangle of the exact basis polynomials, as nested lists of Fractions."""
    rt, dg, hat = ert.HierarchicRT(k), Lagrange(d), Lagrange(1)
    nrt, nd = rt.ndofs, dg.ndofs
    comp = [[b[0] for b in rt.basis], [b[1] for b in rt.basis]]                       # comp[a][i]
    div = [rt.divergence(i) for i in range(nrt)]
    dpsi = [[P.ddx(p) for p in dg.basis], [P.ddy(p) for p in dg.basis]]               # dpsi[a][d]
    monos = [(a, deg - a) for deg in range(k) for a in range(deg, -1, -1)]           # P_{k-1}
    I = P.integrate_triangle
    t = {}
    t["S"] = [[[[I(P.mul(comp[a][i], comp[b][j])) for j in range(nrt)] for i in range(nrt)] for b in range(2)]
              for a in range(2)]
    t["R"] = [[[I(P.mul(comp[a][i], dg.basis[e])) for e in range(nd)] for i in range(nrt)] for a in range(2)]
    t["PP"] = [[I(P.mul(dg.basis[e], dg.basis[g])) for g in range(nd)] for e in range(nd)]
    t["V"] = [[[I(P.mul(hat.basis[v], comp[a][i])) for a in range(2)] for i in range(nrt)] for v in range(3)]
    t["Cdiv"] = [_coeffs(p, monos) for p in div]
    t["Cpsi"] = [_coeffs(p, monos) for p in dg.basis]
    t["Cdpsi"] = [[_coeffs(p, monos) for p in dpsi[a]] for a in range(2)]
    mm = [[I(P.mul(P.monomial(*p), P.monomial(*q))) for q in monos] for p in monos]
    t["MM"] = mm
    nq = len(monos)
    t["GMI"] = P.solve_exact(mm, [[Fraction(int(i == j)) for j in range(nq)] for i in range(nq)])
    t["DV"] = [[I(P.mul(p, P.monomial(*q))) for q in monos] for p in div]
    t["HG"] = [[I(P.mul(p, P.monomial(*q))) for q in monos] for p in dg.basis]
    t["DM"] = [[[I(P.mul(p, P.monomial(*q))) for q in monos] for p in dpsi[a]] for a in range(2)]
    t["F0"] = [[[P.integrate_unit_interval(P.restrict_to_line(p, *ert.FACET_PARAM[f]), j) for j in range(k)]
                for p in dg.basis] for f in range(3)]
    t["monos"] = monos
    return t


@functools.lru_cache(maxsize=None)
def tables(k, d, T):
    t = exact_tables(k, d)
    out = {n: _arr(v, T) for n, v in t.items() if n != "monos"}
    out["monos"] = t["monos"]
    return out


# ---- data ------------------------------------------------------------------------------------------------------------
def seed_of(*key):
    return zlib.crc32("-".join(str(q) for q in key).encode())


def f_osc(r, x, y):
    return np.sin(3.0 * x + r) * np.exp(0.5 * y) + x * y - 0.25 * r


@functools.lru_cache(maxsize=None)
def data(name, k, d, nrhs=3):
    """Random non-equilibrated x, G, f [nrhs, ...], Korn constants in [1, 2], point values of f at the images of the
    rule of degree QDEG, all boundary facets (hole: both loops) and random boundary values; seeded by (name, k, d)."""
    mesh = mesh_of(name)
    rng = np.random.default_rng(seed_of("estimator", name, k, d))
    nrt, nd = k * (k + 2), nd_of(d)
    out = dict(x=rng.standard_normal((nrhs, mesh.ncells * nrt)), G=rng.standard_normal((nrhs, mesh.ncells * nd * 2)),
               f=rng.standard_normal((nrhs, mesh.ncells * nd)), korn=1.0 + rng.random(mesh.ncells),
               bv=rng.standard_normal((nrhs, mesh.ncells * nrt)))
    qp, qw = make_quadrature_triangle(QDEG)
    J = geometry(mesh)[0]
    xq = mesh.x[mesh.cell_nodes[:, 0], :2][:, None, :] + np.einsum("cxa,qa->cqx", J, qp)
    span = np.abs(mesh.x[:, :2]).max()
    out.update(qp=qp, qw=qw, fv=np.stack([f_osc(r, xq[..., 0] / span, xq[..., 1] / span) for r in range(nrhs)]))
    out["facets"] = np.ascontiguousarray(mesh.boundary_facets(), dtype=np.int32)
    for v in out.values():
        v.setflags(write=False)
    return out


# ---- statements ------------------------------------------------------------------------------------------------------
class Statements:
    """Every output of the estimator kernels on one mesh for RT_k with DG_d data, evaluated in T; see the module's
    docstring.  Arguments are single right-hand sides (flat arrays)."""

    def __init__(self, mesh, k, d, T=np.float64):
        self.mesh, self.k, self.d, self.T = mesh, k, d, T
        self.t = tables(k, d, T)
        self.J, self.det, self.adj = geometry(mesh, T)
        self.nrt, self.nd, self.nq = k * (k + 2), nd_of(d), k * (k + 1) // 2
        self.M = np.einsum("cxa,cxb->cab", self.J, self.J) / np.abs(self.det)[:, None, None]
        self.Mabs = np.einsum("cxa,cxb->cab", np.abs(self.J), np.abs(self.J)) / np.abs(self.det)[:, None, None]
        self.sgn = np.where(self.det > 0, T(1), T(-1))

    def _c(self, x):
        return np.asarray(x).astype(self.T).reshape(self.mesh.ncells, self.nrt)

    def _g(self, G):
        return np.asarray(G).astype(self.T).reshape(self.mesh.ncells, self.nd, 2)

    @staticmethod
    def _quad(v, S, M):
        """sum_ab M_ab v^T S_ab v in two stages (the chain: one dot product over j, one over i, one over ab)"""
        u = np.einsum("abij,cj->cabi", S, v)
        w = np.einsum("ci,cabi->cab", v, u)
        return np.einsum("cab,cab->c", M, w)

    # -- || sigma ||^2_T and || sigma - G ||^2_T --------------------------------------------------------------------
    def sig2(self, x, G=None, conforming=False):
        c = self._c(x)
        val, A = self._quad(c, self.t["S"], self.M), self._quad(np.abs(c), np.abs(self.t["S"]), self.Mabs)
        if not conforming:
            return val, A
        g = self._g(G)
        # (sigma, G) = sign(det) sum c_i G_ex J_xa R_aie,  (G, G) = |det| sum G_e . G_g PP_eg
        jg, jga = np.einsum("cxa,cex->cae", self.J, g), np.einsum("cxa,cex->cae", np.abs(self.J), np.abs(g))
        sg = self.sgn * np.einsum("ci,cai->c", c, np.einsum("aie,cae->cai", self.t["R"], jg))
        sga = np.einsum("ci,cai->c", np.abs(c), np.einsum("aie,cae->cai", np.abs(self.t["R"]), jga))
        gg = np.abs(self.det) * np.einsum("cex,cex->c", g, np.einsum("eg,cgx->cex", self.t["PP"], g))
        gga = np.abs(self.det) * np.einsum("cex,cex->c", np.abs(g), np.einsum("eg,cgx->cex", np.abs(self.t["PP"]),
                                                                             np.abs(g)))
        return val - 2 * sg + gg, A + 2 * sga + gga

    # -- divergence of sigma (+ G) in monomial coefficients of the reference cell ----------------------------------------
    def _div_coeffs(self, c, g):
        t = self.t
        co = np.einsum("ci,ip->cp", c, t["Cdiv"]) / self.det[:, None]
        ca = np.einsum("ci,ip->cp", np.abs(c), np.abs(t["Cdiv"])) / np.abs(self.det)[:, None]
        if g is not None:
            Kax = self.adj / self.det[:, None, None]
            co = co + np.einsum("cax,caxp->cp", Kax, np.einsum("cex,aep->caxp", g, t["Cdpsi"]))
            ca = ca + np.einsum("cax,caxp->cp", np.abs(Kax), np.einsum("cex,aep->caxp", np.abs(g), np.abs(t["Cdpsi"])))
        return co, ca

    def _moments_abs(self, c, g, f):
        """abs-sums of the kernel's moments m_q [c, q] (of det J * residual)"""
        t = self.t
        m = np.einsum("ci,iq->cq", np.abs(c), np.abs(t["DV"]))
        if f is not None:
            m = m + np.abs(self.det)[:, None] * np.einsum("ce,eq->cq", np.abs(f), np.abs(t["HG"]))
        if g is not None:
            h = np.einsum("cax,cex->cae", np.abs(self.adj), np.abs(g))
            m = m + np.einsum("cae,aeq->cq", h, np.abs(t["DM"]))
        return m

    def div2(self, x, G, f, conforming=False):
        """|| f - div(sigma + G) ||^2_T (conforming: the total flux is sigma)"""
        c, g = self._c(x), (None if conforming else self._g(G))
        ff = np.asarray(f).astype(self.T).reshape(self.mesh.ncells, self.nd)
        dc, da = self._div_coeffs(c, g)
        r = np.einsum("ce,ep->cp", ff, self.t["Cpsi"]) - dc
        ra = np.einsum("ce,ep->cp", np.abs(ff), np.abs(self.t["Cpsi"])) + da
        ad = np.abs(self.det)
        val = ad * np.einsum("cp,cp->c", r, np.einsum("pq,cq->cp", self.t["MM"], r))
        A = ad * np.einsum("cp,cp->c", ra, np.einsum("pq,cq->cp", self.t["MM"], ra))
        m = self._moments_abs(c, g, ff)
        A_dev = np.einsum("cp,cp->c", m, np.einsum("pq,cq->cp", np.abs(self.t["GMI"]), m)) / ad
        return val, A + A_dev

    # -- oscillation -------------------------------------------------------------------------------------------------
    def h2(self):
        J = self.J
        e = np.stack([J[:, :, 0], J[:, :, 1], J[:, :, 1] - J[:, :, 0]], axis=1)
        return (e * e).sum(axis=2).max(axis=1)

    def oscillation(self, x, G, qp, qw, fv, korn=None):
        T = self.T
        c, g = self._c(x), (None if G is None else self._g(G))
        dc, da = self._div_coeffs(c, g)
        qp, qw = np.asarray(qp).astype(T), np.asarray(qw).astype(T)
        mono = np.stack([qp[:, 0] ** a * qp[:, 1] ** b for a, b in self.t["monos"]], axis=1)      # [q, p]
        fq = np.asarray(fv).astype(T).reshape(self.mesh.ncells, -1)
        r = fq - np.einsum("cp,qp->cq", dc, mono)
        ra = np.abs(fq) + np.einsum("cp,qp->cq", da, mono)
        ck = np.ones(self.mesh.ncells, dtype=T) if korn is None else np.asarray(korn).astype(T)
        pi = T(4) * np.arctan(T(1))
        pre = ck * ck * self.h2() / (pi * pi) * np.abs(self.det)
        m = self._moments_abs(c, g, None)
        rdev = np.abs(fq) + np.einsum("cp,qp->cq", np.einsum("pq,cq->cp", np.abs(self.t["GMI"]), m), mono) \
            / np.abs(self.det)[:, None]
        return pre * np.einsum("q,cq->c", qw, r * r), pre * np.einsum("q,cq->c", qw, ra * ra + rdev * rdev)

    # -- facet moments -------------------------------------------------------------------------------------------------
    def _facet_dofs(self, c, g):
        """[c, lf, j]: facet DOF j of sigma + G on local facet lf (moments of the reference normal flux against s^j),
        and the abs-sum"""
        k = self.k
        mu = c[:, :3 * k].reshape(-1, 3, k).copy()
        mua = np.abs(mu)
        if g is not None:
            n = np.array(ert.FACET_NORMALS, dtype=self.T)                                  # [lf, a]
            nu = np.einsum("cax,la->clx", self.adj, n)
            nua = np.einsum("cax,la->clx", np.abs(self.adj), np.abs(n))
            gn, gna = np.einsum("cex,clx->cle", g, nu), np.einsum("cex,clx->cle", np.abs(g), nua)
            mu = mu + np.einsum("lej,cle->clj", self.t["F0"], gn)
            mua = mua + np.einsum("lej,cle->clj", np.abs(self.t["F0"]), gna)
        return mu, mua

    def jump_moments(self, x, G, conforming=False):
        """[nfacets, k]: moment j of the jump of the outward normal flux of sigma + G against s^j, s the parameter of the
        facet's first cell; 0 on boundary facets.  The device returns the maximum over j of the absolute values."""
        mesh, k, T = self.mesh, self.k, self.T
        mu, mua = self._facet_dofs(self._c(x), None if conforming else self._g(G))
        pf = np.where(np.array(ert.FACET_NORMAL_IS_OUTWARD), T(1), T(-1))
        mu = mu * (self.sgn[:, None] * pf[None, :])[:, :, None]
        off = mesh.facet_cells_offsets
        interior = np.nonzero(np.diff(off) == 2)[0]
        c0, c1 = mesh.facet_cells[off[interior]], mesh.facet_cells[off[interior] + 1]
        l0 = np.argmax(mesh.cell_facets[c0] == interior[:, None], axis=1)
        l1 = np.argmax(mesh.cell_facets[c1] == interior[:, None], axis=1)
        rev = mesh.facet_perm[c0, l0] != mesh.facet_perm[c1, l1]
        B = np.array([[(-1) ** i * comb(j, i) for i in range(k)] for j in range(k)], dtype=T)
        m1, m1a = mu[c1, l1], mua[c1, l1]
        t1 = np.where(rev[:, None], np.einsum("ji,fi->fj", B, m1), m1)
        t1a = np.where(rev[:, None], np.einsum("ji,fi->fj", np.abs(B), m1a), m1a)
        val, A = np.zeros((mesh.nfacets, k), dtype=T), np.zeros((mesh.nfacets, k), dtype=T)
        val[interior], A[interior] = mu[c0, l0] + t1, mua[c0, l0] + t1a
        return val, A

    def boundary_residual(self, x, G, facets, bv=None):
        """[nlist, k]: facet DOF j of sigma + G minus the boundary DOF, seen from the facet's first cell"""
        mesh = self.mesh
        facets = np.asarray(facets, dtype=np.int64)
        mu, mua = self._facet_dofs(self._c(x), None if G is None else self._g(G))
        cells = mesh.facet_cells[mesh.facet_cells_offsets[facets]]
        lf = np.argmax(mesh.cell_facets[cells] == facets[:, None], axis=1)
        val, A = mu[cells, lf], mua[cells, lf]
        if bv is not None:
            b = self._c(bv)[:, :3 * self.k].reshape(-1, 3, self.k)[cells, lf]
            val, A = val - b, A + np.abs(b)
        return val, A

    # -- stress estimator ------------------------------------------------------------------------------------------------
    def stress(self, x2, korn=None, pi_1=1.0):
        """(energy, wsym [ncells], asym [nnodes]) and their abs-sums for the rows x2 [2, ncells * nrt]"""
        T, t, mesh = self.T, self.t, self.mesh
        c = np.asarray(x2).astype(T).reshape(2, mesh.ncells, self.nrt)
        ca, J, Ja = np.abs(c), self.J, np.abs(self.J)

        def form(v, S):
            """int_T of the square of the field sum_ia v[c, i, a] phi_i^a / det J"""
            u = np.einsum("abij,cjb->cia", S, v)
            return np.einsum("cia,cia->c", v, u) / np.abs(self.det)

        S, Sa = t["S"], np.abs(t["S"])
        # sigma_r^x = sum_a J_xa sum_i c_ri phi_i^a / det
        comp = lambda r, x: np.einsum("ca,ci->cia", J[:, x, :], c[r])
        compa = lambda r, x: np.einsum("ca,ci->cia", Ja[:, x, :], ca[r])
        fro = sum(form(comp(r, x), S) for r in range(2) for x in range(2))
        froa = sum(form(compa(r, x), Sa) for r in range(2) for x in range(2))
        tr2, tr2a = form(comp(0, 0) + comp(1, 1), S), form(compa(0, 0) + compa(1, 1), Sa)
        asv, asva = comp(0, 1) - comp(1, 0), compa(0, 1) + compa(1, 0)
        as2, as2a = form(asv, S), form(asva, Sa)
        p = T(pi_1)
        fac = p / (T(2) + T(2) * p)
        energy, energya = T(0.5) * (fro - fac * tr2), T(0.5) * (froa + abs(fac) * tr2a)
        ck = np.ones(mesh.ncells, dtype=T) if korn is None else np.asarray(korn).astype(T)
        wsym, wsyma = T(0.25) * ck * ck * as2, T(0.25) * ck * ck * as2a
        loc = self.sgn[:, None] * np.einsum("cia,via->cv", asv, t["V"])
        loca = np.einsum("cia,via->cv", asva, np.abs(t["V"]))
        asym, asyma = np.zeros(mesh.nnodes, dtype=T), np.zeros(mesh.nnodes, dtype=T)
        np.add.at(asym, mesh.cell_nodes.ravel(), loc.ravel())
        np.add.at(asyma, mesh.cell_nodes.ravel(), loca.ravel())
        return (energy, wsym, asym), (energya, wsyma, asyma)


# ---- rounding counts -----------------------------------------------------------------------------------------------
GEO = 1 + 3 + 1          # a difference of coordinates, the determinant (two products, one difference), its reciprocal


def chain(quantity, k, d, nq=0, valence=0):
    """Roundings along the longest chain of the kernel plus those of the statement, per quantity (see the module's
    docstring for the rule).  nrt = k (k + 2), nd = (d + 1)(d + 2) / 2, nm = k (k + 1) / 2 monomials of P_{k-1}; nq the
    points of the oscillation rule, valence the longest CSR row of the mesh.

    sig2      kernel: geometry GEO, the metric g (2 products, 1 sum, 1 product) 4, a table entry 1, the combination
              g0 S0 + g1 S1 + g2 S2 5, the dot product over j nrt, that over i nrt.  Statement: GEO, J^T J / |det| 4,
              a table entry 1, the three dot products nrt + nrt + 4.
    sig2_ev   adds, on both sides, J^T G 3, a table entry 1, the dot product over (i, e) nrt nd (kernel) or nrt + 2 nd
              (statement), the mass product nd^2 (kernel) or 2 nd + 2 nd, the factors 2 alpha sign, alpha^2 |det| and the
              two additions 6.
    div2      kernel: GEO, adj G 3 and det f 1, a table entry 1, the moment sum 3 + 3 nd (three terms per data node),
              doubled by the square, then GMI m nm, m . (GMI m) nm, the reciprocal product 1.  Statement: GEO, K = adj / det
              1, a table entry 1, the coefficient sums nd + nrt + 4 nd, doubled, then the mass contraction 2 nm and |det| 1.
    osc       kernel: the moments as above without f (3 + 2 nd) + GEO + 4, GMI m nm, the division 1, the value at a point
              nm + 1 (the monomial table entry), doubled by the square; the sum over the points nq + 2 (weight, square), h^2
              5, the factors ck^2 h^2 / pi^2 |det| 6.  Statement: coefficients GEO + 2 + nrt + 4 nd, the value nm + 1 (powers:
              k - 1 more), doubled; nq + 2, 5, 6 + 2 (pi).
    jump      kernel: GEO (the sign only), adj^T N 3, G . nu 3 (with beta), a table entry 1, the sum over the data nodes
              nd + 1, the sign 0, the reversal k (exact binomials), the final addition 1.  Statement: the same chain.
    bres      as jump without the reversal, plus the subtraction of the boundary value 1.
    energy    kernel: GEO, a table entry 1, W: nrt + nrt, prod: 4 terms of 3 products 4 + 3 + 1 (reciprocal), fro / tr2 4
              + 1, the combination 4.  Statement: GEO, the field J c 1 (+ 1 for the sum of two), a table entry 1, the two
              dot products 2 nrt + 2 nrt (over (j, b) and (i, a)), the division 1, sums 4, the combination 4.
    wsym      as energy with ck^2 / 4: 2 more on both sides.
    asym      kernel: J v 3, the product with c and the difference 3, the sum over i 2 nrt, a table entry 1, the sum over
              the row `valence`.  Statement: the field 2, a table entry 1, the dot product 2 nrt, the sign 0, `valence`."""
    nrt, nd, nm = k * (k + 2), nd_of(d), k * (k + 1) // 2
    if quantity == "sig2":
        return (GEO + 4 + 1 + 5 + 2 * nrt) + (GEO + 4 + 1 + 2 * nrt + 4)
    if quantity == "sig2_ev":
        return chain("sig2", k, d) + (3 + 1 + nrt * nd + nd * nd + 6) + (3 + 1 + nrt + 2 * nd + 4 * nd + 6)
    if quantity == "div2":
        return (2 * (GEO + 3 + 1 + 1 + 3 + 3 * nd) + 2 * nm + 1) + (2 * (GEO + 1 + 1 + nd + nrt + 4 * nd) + 2 * nm + 1)
    if quantity == "osc":
        kern = 2 * (GEO + 4 + 3 + 2 * nd + nm + 1 + nm + 1) + nq + 2 + 5 + 6
        stmt = 2 * (GEO + 2 + nrt + 4 * nd + nm + 1 + k - 1) + nq + 2 + 5 + 8
        return kern + stmt
    if quantity == "jump":
        return 2 * (GEO + 3 + 3 + 1 + nd + 1 + k + 1)
    if quantity == "bres":
        return 2 * (GEO + 3 + 3 + 1 + nd + 1 + 1)
    if quantity in ("energy", "wsym"):
        extra = 2 if quantity == "wsym" else 0
        return (GEO + 1 + 2 * nrt + 8 + 5 + 4 + extra) + (GEO + 2 + 1 + 4 * nrt + 1 + 4 + 4 + extra)
    if quantity == "asym":
        return (3 + 3 + 2 * nrt + 1 + valence) + (2 + 1 + 2 * nrt + valence)
    raise KeyError(quantity)


def ratio(diff, bound):
    """max of diff / bound with 0 / 0 = 0 (printed); the assertion is diff <= bound entry by entry"""
    diff, bound = np.asarray(diff, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    if diff.size == 0:
        return 0.0
    return float(np.max(np.where(bound > 0.0, diff / np.where(bound > 0.0, bound, 1.0),
                                 np.where(diff > 0.0, np.inf, 0.0))))


def max_abs_of_moments(device, val, A, c):
    """The device returns max_j |moment_j|; |max_j |a_j| - max_j |b_j|| <= max_j |a_j - b_j|, so the bound of the
    maximum is the largest bound over j.  Returns (|device - max_j |val||, c U max_j A)."""
    ref = np.abs(val).max(axis=1) if val.size else np.zeros(val.shape[0])
    return np.abs(device - ref.astype(np.float64)), c * U * (A.max(axis=1) if A.size else np.zeros(val.shape[0]))


# ---- Korn constants ------------------------------------------------------------------------------------------------
KORN_MESHES = [n for n in MESHES if n not in ("triangle", "right1")]      # those two have patches of one cell: refused
KORN_LAYOUTS = ["dirichlet", "flux_left"]
# roundings of the normalised dot product t = v1 . v2 / (|v1| |v2|), each at most one unit of |t| <= 1 (Cauchy-Schwarz):
# the components of v1 and v2 enter the dot product and a norm (2 + 2), the dot product 2, each norm 2 (sum of squares
# halved by the root, the root), the product of the norms and the division 2.
KORN_T_ROUNDINGS = 4 + 2 + 4 + 2
# acos, the halving, sin, the square, the division and the factor 3, the sum of three: relative roundings of c_K^2
# (a relative rounding of theta changes 2 / sin^2(theta / 2) by theta cot(theta / 2) <= 2 units)
KORN_TAIL_ROUNDINGS = 2 * 2 + 6


def korn_facet_types(mesh, layout):
    """[1, nfacets]: Dirichlet all around, or flux conditions on the boundary facets left of the middle of the mesh"""
    from synthetic import facet_types
    if layout == "dirichlet":
        return facet_types(mesh)
    assert layout == "flux_left"
    mid = 0.5 * (mesh.x[:, 0].min() + mesh.x[:, 0].max())
    return facet_types(mesh, lambda p: p[:, 0] < mid)


def korn_node_mask(name, mesh):
    """None, or the mask of tests/test_gpu_topology.py on `bowtie`: every node but the pinched one"""
    if name != "bowtie":
        return None
    import topology_meshes as tm
    mask = np.ones(mesh.nnodes, dtype=np.uint8)
    mask[tm.pinched_node(mesh)] = 0
    return mask


def korn_restatement(mesh, patches, T=np.longdouble, mask=None):
    """The formula of the oracle (Kim's bound 2 / sin^2(theta_min / 2) on the patch of every node) restated in T on the
    fans `patches` = oracle.build_patches(mesh, ft).  Returns (c_K^2 per node, theta_min per node, amp per node): amp is
    the largest |coordinate| / |v1| met at a boundary patch, whose centre points (centroids, midpoints) are sums of
    coordinates - their rounding is one unit of the COORDINATE, not of the short vector v1 = centre - node."""
    x = mesh.x[:, :2].astype(T)
    pi = T(4) * np.arctan(T(1))
    cks, theta, amp = np.zeros(mesh.nnodes, dtype=T), np.zeros(mesh.nnodes, dtype=T), np.ones(mesh.nnodes)

    def angle(v1, v2):
        return np.arccos((v1 @ v2) / (np.sqrt(v1 @ v1) * np.sqrt(v2 @ v2)))

    def other(facet, node):
        a, b = mesh.facet_nodes[facet]
        return b if a == node else a

    for node in range(mesh.nnodes):
        if mask is not None and not mask[node]:
            continue
        n = int(patches["ncells"][node])
        cells, fcts = patches["cells"][node], patches["fcts"][node]
        if patches["types"][node, 0] == 0:
            th = pi / 2
            for a in range(1, n + 1):
                b = [v for v in mesh.cell_nodes[cells[a]] if v != node]
                v2 = x[b[1]] - x[b[0]]
                th = min(th, angle(x[node] - x[b[0]], v2), angle(x[node] - x[b[1]], -v2))
        else:
            nf = n + 1
            centroid = lambda cell: sum(x[v] / 3 for v in mesh.cell_nodes[cell])
            midpoint = lambda fct: sum(x[v] / 2 for v in mesh.facet_nodes[fct])
            if n % 2 == 0:
                cn = [centroid(cells[n // 2]), centroid(cells[n // 2 + 1]), midpoint(fcts[n // 2])]
            else:
                cn = [midpoint(fcts[nf // 2]), midpoint(fcts[nf // 2 - 1]), centroid(cells[nf // 2])]
            phi = [pi, pi, pi]
            xi = x[node]
            v2 = x[other(fcts[n], node)] - xi
            for i in range(nf):
                nxt = x[other(fcts[i], node)]
                v3 = nxt - xi
                for j in range(3):
                    v1 = cn[j] - xi
                    phi[j] = min(phi[j], angle(v1, v2), angle(v1, v3))
                    big = max(float(np.abs(cn[j]).max()), float(np.abs(xi).max()))
                    amp[node] = max(amp[node], big / float(np.sqrt(v1 @ v1)))
                xi, v2 = nxt, -v3
            th = max(phi)
        theta[node] = th
        cks[node] = 2 / np.sin(th / 2) ** 2
    return cks, theta, amp


def korn_cells(mesh, cks):
    """(gdim + 1) c_K^2 of its three patches per cell"""
    return 3 * cks[mesh.cell_nodes].sum(axis=1)


def korn_tolerance(mesh, cks_node, amp=None):
    """Absolute tolerance per cell of the accumulated squared Korn constants from the conditioning of the formula: the
    relative change of 2 / sin^2(theta / 2) per unit change of the argument t of acos is cot(theta / 2) / sin(theta),
    theta recovered from c_K^2 of the node; t carries KORN_T_ROUNDINGS units, at a boundary patch 6 amp more (the centre
    point: three quotients and two additions, or two products and one addition, in each of two components, on values of
    the size of the coordinates); summed over the three patches of a cell."""
    cks = np.asarray(cks_node, dtype=np.float64)
    ok = cks > 0
    th = 2.0 * np.arcsin(np.sqrt(2.0 / np.where(ok, cks, 2.0)))
    cond = 1.0 / (np.tan(th / 2) * np.sin(th))
    units = KORN_T_ROUNDINGS + (0.0 if amp is None else 6.0 * np.where(np.asarray(amp) > 1.0, amp, 0.0))
    per_node = np.where(ok, cks * (cond * units + KORN_TAIL_ROUNDINGS) * U, 0.0)
    return 3 * per_node[mesh.cell_nodes].sum(axis=1)


_KORN = {}


def korn_reference(oracle, name, layout):
    """(the oracle's accumulated c_K^2 per cell, its c_K^2 per node, the long-double restatement per node, amp per node,
    the tolerance per cell); computed once per (mesh, layout)"""
    if (name, layout) not in _KORN:
        mesh = mesh_of(name)
        ft, mask = korn_facet_types(mesh, layout), korn_node_mask(name, mesh)
        per_node, ref = np.zeros(mesh.nnodes), np.zeros(mesh.ncells)
        for i in (range(mesh.nnodes) if mask is None else np.nonzero(mask)[0]):
            kc = oracle.se_korn(mesh, ft, node_range=(int(i), int(i) + 1))
            per_node[i] = kc.max() / 3
            ref += kc
        if mask is None:
            assert np.array_equal(ref, oracle.se_korn(mesh, ft))
        cks, _, amp = korn_restatement(mesh, oracle.build_patches(mesh, ft), np.longdouble, mask)
        _KORN[(name, layout)] = (ref, per_node, cks, amp, korn_tolerance(mesh, per_node, amp))
    return _KORN[(name, layout)]


# ---- the table of quantities -----------------------------------------------------------------------------------------
CASES = [(n, k, k - 1) for n in MESHES for k in (1, 2, 3, 4)]
LOWDEG = [(k, d) for k in (2, 3, 4) for d in range(k - 1)]
MOMENTS = ("jump", "jump_ev", "bres", "bres_bv", "bres_sigma")       # [n, k] moments: the device returns max_j | . |
OSC = {"osc": (True, True), "osc_nokorn": (True, False), "osc_sigma": (False, True), "osc_sigma_nokorn": (False, False)}
PI_1 = (1.0, 50.0)


def case_id(case):
    return "-".join(str(c) for c in case)


@functools.lru_cache(maxsize=None)
def quantities(name, k, d, T=np.float64, r=0, stress=True):
    """key -> (value, A, c) of every output of the kernels for right-hand side r of data(name, k, d), evaluated in T.
    The stress terms (rows r, r + 1 of x; d plays no part) come with stress=True."""
    mesh, D = mesh_of(name), data(name, k, d)
    st = Statements(mesh, k, d, T)
    x, G, f, bv, korn = D["x"][r], D["G"][r], D["f"][r], D["bv"][r], D["korn"]
    nq, val = D["qw"].size, pm.valence(mesh)
    out = {}
    for ev in (False, True):
        tag = "_ev" if ev else ""
        out["div2" + tag] = st.div2(x, G, f, ev) + (chain("div2", k, d),)
        out["sig2" + tag] = st.sig2(x, G, ev) + (chain("sig2_ev" if ev else "sig2", k, d),)
        out["jump" + tag] = st.jump_moments(x, G, ev) + (chain("jump", k, d),)
    out["bres"] = st.boundary_residual(x, G, D["facets"]) + (chain("bres", k, d),)
    out["bres_bv"] = st.boundary_residual(x, G, D["facets"], bv) + (chain("bres", k, d),)
    out["bres_sigma"] = st.boundary_residual(x, None, D["facets"], bv) + (chain("bres", k, d),)
    for key, (with_g, with_korn) in OSC.items():
        out[key] = st.oscillation(x, G if with_g else None, D["qp"], D["qw"], D["fv"][r], korn if with_korn else None) \
            + (chain("osc", k, d, nq=nq),)
    if stress:
        x2 = D["x"][r:r + 2]
        for p in PI_1:
            (e, w, a), (ea, wa, aa) = st.stress(x2, korn, p)
            out[f"energy{p:g}"] = (e, ea, chain("energy", k, d))
            out[f"wsym{p:g}"] = (w, wa, chain("wsym", k, d))
        out["asym"] = (a, aa, chain("asym", k, d, valence=val))
        (_, w, _), (_, wa, _) = st.stress(x2, None, 1.0)
        out["wsym_nokorn"] = (w, wa, chain("wsym", k, d))
    return out


def deviation(key, got, val, A, c, share=1.0):
    """(|got - value|, share * c U A) per value; for the moments `got` may be the device's max_j | . | or moments"""
    if key in MOMENTS and np.ndim(got) == 1:
        diff, bound = max_abs_of_moments(got, val, A, c)
        return diff, share * bound
    diff = np.abs(np.asarray(got, dtype=np.longdouble) - np.asarray(val, dtype=np.longdouble)).astype(np.float64)
    return diff, share * c * U * np.asarray(A, dtype=np.float64)
