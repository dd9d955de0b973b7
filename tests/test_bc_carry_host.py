"""Boundary conditions across a refinement, as far as they can be checked without a device: the table FB<k> in exact
arithmetic, the numpy statement (dolfinx_eqlb_amd.mesh.refine.carry_facet_types / child_facets,
mesh.transfer.prolong_flux_bc) against moments integrated directly on the child facets, its topology on every mesh of
refine_cases, the condition that those meshes show all six maps of the facet parameter, and the ABI."""

import ctypes as C
import functools
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from refine_cases import NAMES, case

EPS = np.finfo(np.float64).eps
INVALID_ARGUMENT = -1
ENTRIES = ("eqlb_refine_facet_types", "eqlb_refine_child_facets", "eqlb_get_flux_bc_prolong_table",
           "eqlb_refine_prolong_flux_bc", "eqlb_se_carry_boundary", "eqlb_ev_carry_boundary")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEGREES = (1, 2, 3, 4)
# (a, b): positions of the child's low and high local vertex on the parent facet, in the order of the table
MAPS = ((Fraction(0), Fraction(1)), (Fraction(1), Fraction(0)), (Fraction(0), Fraction(1, 2)),
        (Fraction(1, 2), Fraction(1)), (Fraction(1, 2), Fraction(0)), (Fraction(1), Fraction(1, 2)))


@functools.lru_cache(maxsize=None)
def refined(name):
    """(mesh, mesh2, parent_cell, node_parent_facet, parent_facet) of a case of refine_cases by the numpy statement."""
    from dolfinx_eqlb_amd.mesh import create_mesh, parent_facets, refine_longest_edge
    mesh, marked = case(name)
    x2, cells2, pc, npf = refine_longest_edge(mesh, marked)
    mesh2 = create_mesh(x2, cells2)
    return mesh, mesh2, pc, npf, parent_facets(mesh, npf, mesh2)


def identity(k):
    return tuple(tuple(Fraction(int(i == j)) for i in range(k)) for j in range(k))


def matmul(A, B):
    return tuple(tuple(sum((A[j][n] * B[n][i] for n in range(len(B))), Fraction(0)) for i in range(len(B[0])))
                 for j in range(len(A)))


def monomial_integral(n, a, b):
    """int_a^b s^n ds as a Fraction."""
    return (b ** (n + 1) - a ** (n + 1)) / (n + 1)


# ------------------------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize("k", DEGREES)
def test_tables_in_exact_arithmetic(k):
    from dolfinx_eqlb_amd.mesh.transfer import flux_bc_table, flux_bc_table_exact
    FB = flux_bc_table_exact(k)
    assert len(FB) == 6 and all(len(m) == k and all(len(r) == k for r in m) for m in FB)
    assert all(isinstance(v, Fraction) for m in FB for r in m for v in r)
    assert FB[0] == identity(k)
    assert matmul(FB[1], FB[1]) == identity(k)
    # FB[2], FB[3] by an independent construction: the parent DOFs of the monomial s^n are the moments
    # d_i = 1 / (n + i + 1); its moments on the half [a, b] against the child parameter t = (s - a) / (b - a) are
    # int_a^b s^n ((s - a) / (b - a))^j ds - in Fractions from the antiderivatives of the powers of s (the nodes of a
    # Gauss-Legendre rule are irrational), and below in doubles from the rule itself
    from math import comb
    for m in (2, 3):
        a, b = MAPS[m]
        for n in range(k):
            d = [Fraction(1, n + i + 1) for i in range(k)]
            for j in range(k):
                # ((s - a) / (b - a))^j = sum_r C(j, r) s^r (-a)^(j - r) / (b - a)^j
                want = sum((comb(j, r) * (-a) ** (j - r) * monomial_integral(n + r, a, b) for r in range(j + 1)),
                           Fraction(0)) / (b - a) ** j
                got = sum((FB[m][j][i] * d[i] for i in range(k)), Fraction(0))
                assert got == want, (k, m, n, j)
    # and numerically, with the rule itself: 8 points integrate degree 15 >= 2 (k - 1) exactly
    x, w = np.polynomial.legendre.leggauss(8)
    t, w = 0.5 * (x + 1.0), 0.5 * w
    Tf = flux_bc_table(k)
    for m in (2, 3):
        a, b = float(MAPS[m][0]), float(MAPS[m][1])
        for n in range(k):
            d = np.array([1.0 / (n + i + 1) for i in range(k)])
            direct = np.array([(b - a) * np.sum(w * (a + (b - a) * t) ** n * t ** j) for j in range(k)])
            assert np.abs(Tf[m] @ d - direct).max() <= 64 * EPS * np.abs(Tf[m]).sum(axis=1).max()
    # mass is kept: the two halves add up to the whole
    e0 = tuple(Fraction(int(i == 0)) for i in range(k))
    assert tuple(x + y for x, y in zip(FB[2][0], FB[3][0])) == e0
    assert tuple(x + y for x, y in zip(FB[4][0], FB[5][0])) == e0
    if k == 1:
        assert all(v in (Fraction(1), Fraction(1, 2)) for m in FB for r in m for v in r)
    # rounded once
    assert np.array_equal(Tf, np.array([[[float(v) for v in r] for r in m] for m in FB]))


def test_largest_entry_is_15():
    from dolfinx_eqlb_amd.mesh.transfer import flux_bc_table_exact
    big = {k: max(abs(v) for m in flux_bc_table_exact(k) for r in m for v in r) for k in DEGREES}
    assert max(big.values()) == 15 and big[4] == 15 and big[1] == 1, big


@pytest.mark.parametrize("k", DEGREES)
def test_library_table_equals_the_generator(k):
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.mesh import flux_bc_table
    got = cpp.get_flux_bc_prolong_table(k)
    assert got.shape == (6, k, k) and np.array_equal(got, flux_bc_table(k))
    # the committed header is what the generator writes
    header = open(os.path.join(ROOT, "dolfinx_eqlb_amd", "csrc", "eqlb_tables_gen.h")).read()
    body = re.search(r"struct FluxBcProlong<%d> \{\s*static constexpr double FB\[%d\] = \{([^}]*)\}" % (k, 6 * k * k),
                     header).group(1)
    assert np.array_equal(np.array([float(v) for v in body.split(",")]), flux_bc_table(k).ravel())


def test_table_refusals():
    from dolfinx_eqlb_amd import cpp
    L = cpp.lib()
    out = np.full(96, 7.0)
    p = out.ctypes.data_as(C.c_void_p)
    for k, ptr, cap in ((0, p, 96), (5, p, 96), (2, None, 96), (2, p, 23)):
        assert L.eqlb_get_flux_bc_prolong_table(C.c_int32(k), ptr, C.c_int32(cap)) == INVALID_ARGUMENT
        assert "eqlb_get_flux_bc_prolong_table" in L.eqlb_last_error().decode()
    assert np.all(out == 7.0)
    assert L.eqlb_get_flux_bc_prolong_table(C.c_int32(2), p, C.c_int32(24)) == 24   # the next valid call works
    with pytest.raises(RuntimeError, match="outside 1 ... 4"):
        cpp.get_flux_bc_prolong_table(5)


# ------------------------------------------------------------------------------- statement against direct moments
NPOLY = 200


@pytest.mark.parametrize("k", DEGREES)
def test_statement_against_moments_integrated_on_the_child(k):
    """Random g in P_{k-1} (monomial coefficients), random |E|, every map: the parent DOFs |E| int g s^i by an 8-point
    Gauss rule, carried by the statement, against |beta| |E| int g(alpha + beta t) t^j by the same rule on the child.

    Bound, in units of u = eps / 2 and with G(s) = sum_n |c_n| s^n:
      a moment sum_q w_q g(s_q) s_q^j |E|: g by monomials (at most 2k roundings against G), s^j, the weight and the
      product (j + 1 <= k), 7 additions, the scale (1), the rounded nodes and weights of the rule (a relative 2u in
      every s of s^(n+j), n + j <= 2k - 2: at most 4k, and 2 for the weight): N = 7k + 10 roundings against
      D_j = |E| sum_q w_q G(s_q) s_q^j;
      on the child also s = alpha + beta t (2 roundings in a value >= 1/2 of |alpha| + |beta| t, in every one of the
      n <= k - 1 factors: at most 4k): N2 = 11k + 10 against D2_j = |beta| |E| sum_q w_q G(s(t_q)) t_q^j;
      the statement: the errors of the parent DOFs through |FB|, k roundings of the k products and k - 1 sums and one of
      the table entry against A_j <= sum_i |FB_ji| D_i.
    |carried - direct| <= u ((N + k + 1) sum_i |FB_ji| D_i + N2 D2_j); with the margin 2 that is eps (...).
    Measured: worst |carried - direct| = 4.6e-15 max|parent DOF| (k = 3), 0.05 of the bound (k = 2), over 200
    polynomials per (k, map)."""
    from dolfinx_eqlb_amd.mesh.transfer import apply_flux_bc_maps, flux_bc_table
    rng = np.random.default_rng(100 + k)
    x, w = np.polynomial.legendre.leggauss(8)
    t, w = 0.5 * (x + 1.0), 0.5 * w
    T = flux_bc_table(k)
    powers = np.arange(k)
    worst, worst_rel = 0.0, 0.0
    for m in range(6):
        alpha, beta = float(MAPS[m][0]), float(MAPS[m][1] - MAPS[m][0])
        coef = rng.standard_normal((NPOLY, k))
        E = 10.0 ** rng.uniform(-3, 3, NPOLY)

        def g(s):            # [NPOLY, nq]
            return (coef[:, :, None] * s[None, None, :] ** powers[None, :, None]).sum(axis=1)

        def G(s):
            return (np.abs(coef)[:, :, None] * s[None, None, :] ** powers[None, :, None]).sum(axis=1)

        mom = t[None, :] ** powers[:, None]                               # [k, nq]
        parent = E[:, None] * ((w[None, :] * g(t)) @ mom.T)               # [NPOLY, k]
        D = E[:, None] * ((w[None, :] * G(t)) @ mom.T)
        s_child = alpha + beta * t
        direct = abs(beta) * E[:, None] * ((w[None, :] * g(s_child)) @ mom.T)
        D2 = abs(beta) * E[:, None] * ((w[None, :] * G(s_child)) @ mom.T)
        carried, A = apply_flux_bc_maps(k, np.full(NPOLY, m), parent, np.ones(NPOLY))
        assert np.all(A <= (1 + 100 * EPS) * (D @ np.abs(T[m]).T))
        bound = EPS * ((8 * k + 11) * (D @ np.abs(T[m]).T) + (11 * k + 10) * D2)
        err = np.abs(carried - direct)
        worst = max(worst, float((err / bound).max()))
        worst_rel = max(worst_rel, float((err.max(axis=1) / np.abs(parent).max(axis=1)).max()))
        assert np.all(err <= bound), (k, m, float((err / bound).max()))
        if m == 0:
            assert np.array_equal(carried, parent)                         # the whole, equally directed facet
        if k == 1:
            assert np.array_equal(carried, (1.0 if m < 2 else 0.5) * parent)
    print(f"  k = {k}: worst error / bound {worst:.3f}, worst error / max|parent DOF| {worst_rel:.2e}")


# ------------------------------------------------------------------------------------------------------ topology
@pytest.mark.parametrize("name", NAMES)
def test_child_facets_and_parent_facets_are_inverse(name):
    from dolfinx_eqlb_amd.mesh import child_facets
    mesh, mesh2, pc, npf, pf = refined(name)
    ch = child_facets(mesh, npf, mesh2)
    assert ch.shape == (mesh.nfacets, 2) and ch.dtype == np.int32
    assert np.all(ch[:, 0] >= 0)
    cut = np.zeros(mesh.nfacets, dtype=bool)
    cut[npf] = True
    assert np.array_equal(ch[:, 1] >= 0, cut)
    # parent of every child is the facet; every facet with a parent is a child of it
    for col in (0, 1):
        has = ch[:, col] >= 0
        assert np.array_equal(pf[ch[has, col]], np.nonzero(has)[0])
    listed = ch[ch >= 0]
    assert np.unique(listed).size == listed.size
    assert np.array_equal(np.sort(listed), np.nonzero(pf >= 0)[0])
    # a sub-list in any order, with repeats
    pick = np.random.default_rng(3).integers(0, mesh.nfacets, 17)
    assert np.array_equal(child_facets(mesh, npf, mesh2, pick), ch[pick])
    with pytest.raises(ValueError, match="outside"):
        child_facets(mesh, npf, mesh2, [mesh.nfacets])
    # the node pairs of the statement
    lo, hi = mesh.facet_nodes.min(axis=1), mesh.facet_nodes.max(axis=1)
    new_node = np.full(mesh.nfacets, -1)
    new_node[npf] = mesh.nnodes + np.arange(npf.size)
    fn2 = np.sort(mesh2.facet_nodes, axis=1)
    assert np.array_equal(fn2[ch[~cut, 0]], np.stack([lo[~cut], hi[~cut]], axis=1))
    assert np.array_equal(fn2[ch[cut, 0]], np.stack([lo[cut], new_node[cut]], axis=1))
    assert np.array_equal(fn2[ch[cut, 1]], np.stack([hi[cut], new_node[cut]], axis=1))


@pytest.mark.parametrize("name", NAMES)
def test_boundary_stays_boundary_and_types_cover_it(name):
    from dolfinx_eqlb_amd.mesh import carry_facet_types, child_facets
    from synthetic import facet_types
    mesh, mesh2, pc, npf, pf = refined(name)
    ncell2 = np.diff(mesh2.facet_cells_offsets)
    bf = mesh.boundary_facets()
    ch = child_facets(mesh, npf, mesh2, bf)
    assert np.all(ncell2[ch[ch >= 0]] == 1)
    assert np.array_equal(np.sort(ch[ch >= 0]), mesh2.boundary_facets())
    ft = facet_types(mesh, lambda p: p[:, 0] + p[:, 1] > 0.9, nrhs=2)
    ft[1, bf] = 3 - ft[1, bf]
    ft2 = carry_facet_types(ft, pf)
    assert ft2.shape == (2, mesh2.nfacets) and ft2.dtype == np.int8
    assert np.all(ft2[:, ncell2 == 1] > 0) and np.all(ft2[:, ncell2 == 2] == 0)
    for r in range(2):
        for f in bf:
            kids = ch[np.nonzero(bf == f)[0][0]]
            assert np.all(ft2[r, kids[kids >= 0]] == ft[r, f])
    assert np.array_equal(carry_facet_types(ft[0], pf), ft2[0])
    # a value outside 0 ... 2 is copied as it is
    odd = ft.copy()
    odd[0, bf[0]] = 9
    assert np.count_nonzero(carry_facet_types(odd, pf)[0] == 9) == np.count_nonzero(ch[0] >= 0)


# ----------------------------------------------------------------------------------------------------- condition
COUNTED = {0: 718, 1: 188, 2: 64, 3: 64, 4: 27, 5: 27}


def test_the_cases_show_all_six_maps_on_boundary_facets():
    from dolfinx_eqlb_amd.mesh.transfer import FLUX_BC_MAPS, flux_bc_maps
    assert FLUX_BC_MAPS == tuple((int(2 * a), int(2 * b)) for a, b in MAPS)
    counts = np.zeros(6, dtype=np.int64)
    per_case = {}
    for name in NAMES:
        mesh, mesh2, pc, npf, pf = refined(name)
        bf2 = mesh2.boundary_facets()
        C2, l2, P, l, m = flux_bc_maps(mesh, mesh2, pc, npf, bf2)
        assert np.array_equal(P, pc[C2]) and np.array_equal(mesh2.cell_facets[C2, l2], bf2)
        assert np.array_equal(mesh.cell_facets[P, l], pf[bf2])
        # whole facets are unbisected parents, halves are children of a bisected one
        cut = np.zeros(mesh.nfacets, dtype=bool)
        cut[npf] = True
        assert np.array_equal(m >= 2, cut[pf[bf2]])
        per_case[name] = np.bincount(m, minlength=6)
        counts += per_case[name]
    print("  maps on boundary facets:", dict(enumerate(counts.tolist())))
    assert np.all(counts > 0)
    assert dict(enumerate(counts.tolist())) == COUNTED
    assert np.count_nonzero(per_case["right1"]) == 5


@pytest.mark.parametrize("name", ["right1", "sq3_all", "lshape"])
def test_statement_on_a_mesh(name):
    """The gather of the statement: a table that holds the facet id and DOF number comes back through the maps;
    whole, equally directed facets carry their DOFs bit for bit; k = 1 is exact; the refusals name the entry."""
    from dolfinx_eqlb_amd.mesh import flux_bc_table, prolong_flux_bc
    from dolfinx_eqlb_amd.mesh.transfer import flux_bc_maps
    mesh, mesh2, pc, npf, pf = refined(name)
    bf2 = mesh2.boundary_facets()
    rng = np.random.default_rng(5)
    for k in DEGREES:
        nrt = k * (k + 2)
        bv = rng.standard_normal((3, mesh.ncells * nrt))
        C2, l2, P, l, m = flux_bc_maps(mesh, mesh2, pc, npf, bf2)
        got, A = prolong_flux_bc(mesh, mesh2, pc, npf, k, bv, bf2, return_abs=True)
        assert got.shape == A.shape == (3, bf2.size, k)
        d = bv.reshape(3, mesh.ncells, nrt)[:, P[:, None], l[:, None] * k + np.arange(k)[None, :]]
        sigma = np.where(l2 == 1, 1.0, -1.0) * np.where(l == 1, 1.0, -1.0)
        T = flux_bc_table(k)
        ref = sigma[None, :, None] * np.einsum("nji,rni->rnj", T[m], d)
        assert np.all(np.abs(got - ref) <= 2 * k * EPS * A)
        whole = m == 0
        assert np.array_equal(got[:, whole], sigma[None, whole, None] * d[:, whole])
        assert np.array_equal(prolong_flux_bc(mesh, mesh2, pc, npf, k, bv[1], bf2), got[1])
    interior = int(np.nonzero(np.diff(mesh2.facet_cells_offsets) == 2)[0][0])
    for bad, words in ((mesh2.nfacets, "is no facet of the refined mesh"), (-1, "is no facet of the refined mesh"),
                       (interior, "lies between two cells")):
        with pytest.raises(ValueError, match=r"facets2\[1\] = %d %s" % (bad, words)):
            prolong_flux_bc(mesh, mesh2, pc, npf, 1, np.zeros(mesh.ncells * 3), [bf2[0], bad])


# ----------------------------------------------------------------------------------------------------------- ABI
def test_entries_are_declared_exported_and_bound():
    from dolfinx_eqlb_amd import cpp
    header = open(os.path.join(ROOT, "include", "eqlb.h")).read()
    L = cpp.lib()
    for name in ENTRIES:
        assert re.search(r"^int\s+" + name + r"\(", header, flags=re.M), name
        assert name in cpp.EXPORTED_SYMBOLS, name
        assert hasattr(L, name), name
    assert "the flux-boundary DOF" not in header
    for name in ("facet_types_raw", "child_facets_raw", "prolong_flux_bc_raw"):
        assert hasattr(cpp.RefinePlan, name), name
    for name in ("facet_types", "child_facets", "prolong_flux_bc"):
        assert hasattr(cpp.Refinement, name), name
    assert hasattr(cpp, "get_flux_bc_prolong_table")
    for cls in (cpp.SemiExplicitEquilibrator, cpp.ConstrainedMinEquilibrator):
        assert hasattr(cls, "carry_boundary")
    from dolfinx_eqlb_amd import _cpp
    for name in ("facet_types", "child_facets", "prolong_flux_bc"):
        assert hasattr(_cpp.Transfer, name), name
    from dolfinx_eqlb_amd.eqlb.FluxEqlbEV import FluxEqlbEV
    from dolfinx_eqlb_amd.eqlb.FluxEqlbSE import FluxEqlbSE
    assert hasattr(FluxEqlbSE, "refined") and hasattr(FluxEqlbEV, "refined")


def test_statement_is_exported_from_the_mesh_package():
    from dolfinx_eqlb_amd import mesh
    from dolfinx_eqlb_amd.mesh import refine, transfer
    for name in ("carry_facet_types", "child_facets"):
        assert getattr(mesh, name) is getattr(refine, name), name
    for name in ("flux_bc_table_exact", "flux_bc_table", "prolong_flux_bc"):
        assert getattr(mesh, name) is getattr(transfer, name), name


def test_a_closed_plan_raises_as_prolong_does():
    from dolfinx_eqlb_amd import cpp
    r = cpp.Refinement(None, None, None, None, {"nnodes2": 0, "ncells2": 0})
    for call in (lambda: r.facet_types(np.zeros(3, dtype=np.int8)), lambda: r.child_facets([0]),
                 lambda: r.prolong_flux_bc(1, np.zeros(3), [0])):
        with pytest.raises(RuntimeError, match="keep_plan=True"):
            call()
    eq = cpp.SemiExplicitEquilibrator.__new__(cpp.SemiExplicitEquilibrator)
    eq._h = C.c_void_p()
    with pytest.raises(RuntimeError, match="keep_plan=True"):
        eq.carry_boundary(eq, r)


def test_null_arguments_are_refused():
    from dolfinx_eqlb_amd import cpp
    L = cpp.lib()
    idx = np.full(12, 3, dtype=np.int32)
    typ = np.full(12, 1, dtype=np.int8)
    val = np.full(12, 7.0)
    pi, pt, pv = (a.ctypes.data_as(C.c_void_p) for a in (idx, typ, val))
    host, one = C.c_int32(0), C.c_int32(1)
    fake = C.c_void_p(0x5EED5EED)   # never dereferenced: the null argument is found first

    for plan, refined_, ft, ft2 in ((None, fake, pt, pt), (fake, None, pt, pt), (None, None, None, pt),
                                    (None, None, pt, None)):
        assert L.eqlb_refine_facet_types(plan, refined_, one, ft, ft2, host, None) == INVALID_ARGUMENT
        assert "eqlb_refine_facet_types" in L.eqlb_last_error().decode()
    for plan, refined_ in ((None, fake), (fake, None)):
        assert L.eqlb_refine_child_facets(plan, refined_, one, pi, pi, host, None) == INVALID_ARGUMENT
        assert "eqlb_refine_child_facets" in L.eqlb_last_error().decode()
    for plan, refined_, bv in ((None, fake, pv), (fake, None, pv), (None, None, None)):
        st = L.eqlb_refine_prolong_flux_bc(plan, refined_, one, one, bv, one, pi, pv, host, None)
        assert st == INVALID_ARGUMENT
        assert "eqlb_refine_prolong_flux_bc" in L.eqlb_last_error().decode()
    for fn, name in ((L.eqlb_se_carry_boundary, "eqlb_se_carry_boundary"),
                     (L.eqlb_ev_carry_boundary, "eqlb_ev_carry_boundary")):
        for old, plan, fresh in ((None, fake, fake), (None, None, None)):
            assert fn(old, plan, fresh, None, None) == INVALID_ARGUMENT
            assert name in L.eqlb_last_error().decode()
    assert np.all(idx == 3) and np.all(typ == 1) and np.all(val == 7.0)
