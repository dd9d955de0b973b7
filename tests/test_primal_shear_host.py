"""The cell-wise shear modulus of the elasticity chain as far as it can be checked without a device: the numpy statement
(lsolver.primal.ElasticityOperator.set_shear) against the Galerkin matrix with mu_T inside the integral, the exact
cases mu = 1 and mu = 4, the refusals, the statement of the estimate (check_eqlb_conditions.stress_estimator_terms with
cell_pi1 / mu / cell_mu), the entries in header, library and bindings, and the guaranteed upper bound on the bimaterial
square of tests/shear_cases.py with the oracle."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import elasticity_cases as ec
import shear_cases as sc
from dolfinx_eqlb_amd.eqlb import check_eqlb_conditions as chk
from dolfinx_eqlb_amd.lsolver import primal
from dolfinx_eqlb_amd.mesh import create_unit_square
from primal_cases import ratio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = ec.U
MESH = create_unit_square(4, shuffle_seed=3, perturb=0.15)
VALUES = np.array([1e-3, 0.7, 1e3])


def three_valued(ncells, seed=11):
    """cell-wise mu with three distinct values six orders of magnitude apart"""
    return VALUES[np.random.default_rng(seed).integers(0, 3, size=ncells)]


# ---- the statement against the assembled matrix ----------------------------------------------------------------------------
@pytest.mark.parametrize("react", [False, True])
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_statement_equals_the_operator_assembled_with_mu_inside_the_integral(p, react):
    """|statement - assembled| <= 2^-53 (ts |statement|-sum + ta |assembled|-sum), compared the way
    elasticity_cases.check_statement compares the operator without the term, with the roundings the modulus adds to
    elasticity_cases.chain_terms: the statement takes ONE more product, mu_T v (ts + 1); the assembled side one product
    v * A_v per value and the sums of the three restricted matrices in an entry that cells of different values share
    (ta + 3).  With a reaction term (+ 1, + 1 as reaction_cases.chain_terms counts it) the mass part is not scaled."""
    from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
    import reaction_cases as rc
    mesh = MESH
    rng = np.random.default_rng(17 + p)
    pi1, mu = ec.pi1_of(mesh.ncells), three_valued(mesh.ncells)
    assert np.unique(mu).size == 3
    op = primal.ElasticityOperator(mesh, p, cell_pi1=pi1)
    op.set_shear(cell_mu=mu)
    A, Aabs, nvalues = sc.assemble_mu(mesh, p, pi1, mu)
    valence = int(np.diff(mesh.node_cells_offsets).max())
    ts, ta = ec.chain_terms(p, valence, make_quadrature_triangle(2 * p + 4)[1].size)
    ts, ta = ts + 1, ta + nvalues
    if react:
        c = rc.c_of(mesh.ncells)
        op.set_reaction(cell_c=c)
        M, Mabs = rc.assemble_mass(mesh, p, c, 2)
        A, Aabs, ts, ta = A + M, Aabs + Mabs, ts + 1, ta + 1
    u = rng.standard_normal(2 * op.ndofs)
    y, yabs = op.apply(u, return_abs=True)
    diff, bound = np.abs(y - A @ u), U * (ts * yabs + ta * (Aabs @ np.abs(u)))
    print(f"p={p} react={react}: apply max |diff| / bound = {ratio(diff, bound):.3f} (terms {(ts, ta)})")
    assert np.all(diff <= bound)
    dg, dabs = op.diagonal(return_abs=True)
    diff, bound = np.abs(dg - A.diagonal()), U * (ts * dabs + ta * Aabs.diagonal())
    print(f"p={p} react={react}: diagonal max |diff| / bound = {ratio(diff, bound):.3f}")
    assert np.all(diff <= bound) and np.all(dg > 0.0)
    # the modulus is in the operator: without it the statement misses the assembled matrix by far more than the bound
    op.set_shear()
    assert not np.all(np.abs(op.apply(u) - A @ u) <= bound.max())
    # the load is unchanged, the residual follows apply
    op.set_shear(cell_mu=mu)
    f = rng.standard_normal((2, mesh.ncells * 3))
    b = op.load(1, f)
    assert np.array_equal(b, primal.ElasticityOperator(mesh, p, cell_pi1=pi1).load(1, f))
    bf = mesh.boundary_facets()
    op.set_dirichlet(bf, bf)
    r = op.residual(b, u)
    assert np.array_equal(r[~op.fixed], (b - y)[~op.fixed]) and np.all(r[op.fixed] == 0.0)


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_one_gives_the_bits_without_the_term_and_four_gives_four_times_them(p):
    mesh = MESH
    rng = np.random.default_rng(p)
    pi1 = ec.pi1_of(mesh.ncells)
    op, plain = primal.ElasticityOperator(mesh, p, cell_pi1=pi1), primal.ElasticityOperator(mesh, p, cell_pi1=pi1)
    u = rng.standard_normal(2 * op.ndofs)
    y0, d0 = plain.apply(u), plain.diagonal()
    op.set_shear(cell_mu=sc_mu(mesh.ncells))
    assert not np.array_equal(op.apply(u), y0)
    op.set_shear(1.0)
    assert op.mu is None
    assert np.array_equal(op.apply(u).view(np.int64), y0.view(np.int64))
    assert np.array_equal(op.diagonal().view(np.int64), d0.view(np.int64))
    for kw in (dict(mu=4.0), dict(cell_mu=np.full(mesh.ncells, 4.0))):
        op.set_shear(**kw)                         # a power of two: exact
        assert np.array_equal(op.apply(u).view(np.int64), (4.0 * y0).view(np.int64))
        assert np.array_equal(op.diagonal().view(np.int64), (4.0 * d0).view(np.int64))
    # the reaction term is not scaled: (4 v) + wm m
    op.set_reaction(2.5)
    plain.set_reaction(2.5)
    wm_m = plain.wm[:, None] * primal._sum_products(plain.Mass, u.reshape(-1, 2)[plain.cell_dofs][:, :, 0])[0]
    got = op.cell_product(u)[:, :, 0]
    op.set_reaction()
    assert np.array_equal(got.view(np.int64), (op.cell_product(u)[:, :, 0] + wm_m).view(np.int64))
    op.set_shear()
    assert np.array_equal(op.apply(u).view(np.int64), y0.view(np.int64))


def sc_mu(ncells, seed=41):
    return 10.0 ** (-3.0 + 6.0 * np.random.default_rng(seed).random(ncells))


def test_refusals_of_the_statement():
    op = primal.ElasticityOperator(MESH, 2)
    n = MESH.ncells
    op.set_shear(2.0)
    for value in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="set_shear: mu = "):
            op.set_shear(value)
        bad = np.ones(n)
        bad[6] = value
        with pytest.raises(ValueError, match=r"set_shear: cell_mu\[6\] = "):
            op.set_shear(cell_mu=bad)
        assert np.array_equal(op.mu, np.full(n, 2.0))              # left as it was
    with pytest.raises(ValueError, match="cell_mu \\[ncells\\] expected"):
        op.set_shear(cell_mu=np.ones(n + 1))


# ---- the statement of the estimate -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3])
def test_estimator_terms_take_cell_pi1_and_divide_by_mu(k):
    mesh = MESH
    rng = np.random.default_rng(k)
    x = rng.standard_normal((2, mesh.ncells * k * (k + 2)))
    korn = 1.0 + rng.random(mesh.ncells)
    values = np.array([0.5, 1.0, 40.0])
    pick = rng.integers(0, 3, size=mesh.ncells)
    pi1, mu = values[pick], sc_mu(mesh.ncells)
    e0, w0 = chk.stress_estimator_terms(mesh, k, x, korn, 1.0)
    for out in (chk.stress_estimator_terms(mesh, k, x, korn), chk.stress_estimator_terms(mesh, k, x, korn, 1.0, None, 1.0)):
        assert np.array_equal(out[0], e0) and np.array_equal(out[1], w0)        # the defaults give today's values
    e, w = chk.stress_estimator_terms(mesh, k, x, korn, cell_pi1=pi1, cell_mu=mu)
    for i, v in enumerate(values):
        ev, wv = chk.stress_estimator_terms(mesh, k, x, korn, float(v))
        sel = pick == i
        assert np.array_equal(e[sel], (ev / mu)[sel]) and np.array_equal(w[sel], (wv / mu)[sel])
    # a global constant mu = m: the terms of mu = 1 divided by m
    e4, w4 = chk.stress_estimator_terms(mesh, k, x, korn, 1.0, mu=4.0)
    assert np.array_equal(e4, e0 / 4.0) and np.array_equal(w4, w0 / 4.0)
    with pytest.raises(ValueError, match="mu"):
        chk.stress_estimator_terms(mesh, k, x, korn, mu=0.0)


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    import inspect
    from dolfinx_eqlb_amd import _cpp, cpp, lsolver
    header = open(os.path.join(ROOT, "include", "eqlb.h")).read()
    L = cpp.lib()
    for name in ("eqlb_elasticity_set_shear", "eqlb_primal_stress_dg_mu", "eqlb_se_estimate_stress_mu"):
        assert re.search(r"^int\s+" + name + r"\(", header, flags=re.M), name
        assert name in cpp.EXPORTED_SYMBOLS and hasattr(L, name), name
    assert "eqlb_hierarchy_set_coarse(handle, 1, ...) has to be called again" in header
    assert hasattr(cpp.PrimalElasticity, "set_shear") and hasattr(cpp.PrimalElasticity, "set_shear_raw")
    assert not hasattr(cpp.PrimalPoisson, "set_shear")
    assert hasattr(_cpp.PrimalElasticity, "set_shear")
    for fn, names in ((cpp.primal_stress_dg, ("mu", "cell_mu")), (cpp.estimate_stress, ("cell_pi1", "mu", "cell_mu")),
                      (chk.stress_estimator_terms, ("cell_pi1", "mu", "cell_mu"))):
        par = inspect.signature(fn).parameters
        for nm in names:
            assert nm in par and par[nm].default in (None, 1.0), (fn.__name__, nm)
    fields = {f.name: f.default for f in lsolver.PrimalStress.__dataclass_fields__.values()}
    assert fields["mu"] == 1.0 and fields["cell_mu"] is None


def test_abi_refuses_bad_arguments_before_the_device():
    from dolfinx_eqlb_amd import cpp
    L = cpp.lib()
    fake = C.c_void_p(0x5EED5EED)   # never dereferenced: the refusal comes first
    one = np.ones(4)
    pv = one.ctypes.data_as(C.c_void_p)

    def refused(st, *words):
        assert st == -1
        msg = L.eqlb_last_error().decode()
        for w in words:
            assert w in msg, (w, msg)

    ss = L.eqlb_elasticity_set_shear
    refused(ss(None, C.c_double(2.0), None, C.c_int32(0), None), "eqlb_elasticity_set_shear", "null handle")
    refused(ss(fake, C.c_double(2.0), None, C.c_int32(9), None), "eqlb_elasticity_set_shear", "memory space")
    for v in (0.0, -3.0, float("nan"), float("inf")):
        refused(ss(fake, C.c_double(v), None, C.c_int32(0), None), "eqlb_elasticity_set_shear", "mu =")
        refused(L.eqlb_primal_stress_dg_mu(fake, C.c_int32(2), C.c_int32(1), pv, C.c_int64(4), pv, C.c_double(1.0), None,
                                           C.c_double(v), None, None, pv, C.c_int32(0), None),
                "eqlb_primal_stress_dg_mu", "mu =")
        refused(L.eqlb_se_estimate_stress_mu(fake, C.c_int32(2), pv, None, C.c_double(1.0), None, C.c_double(v), None,
                                             pv, pv, None, C.c_int32(0), None), "eqlb_se_estimate_stress_mu", "mu =")
    refused(L.eqlb_primal_stress_dg_mu(fake, C.c_int32(5), C.c_int32(1), pv, C.c_int64(4), pv, C.c_double(1.0), None,
                                       C.c_double(2.0), None, None, pv, C.c_int32(0), None),
            "eqlb_primal_stress_dg_mu", "degrees")
    refused(L.eqlb_se_estimate_stress_mu(None, C.c_int32(2), pv, None, C.c_double(1.0), None, C.c_double(2.0), None,
                                         pv, pv, None, C.c_int32(0), None), "eqlb_se_estimate_stress_mu", "invalid")
    assert np.all(one == 1.0)


# ---- the bound on the bimaterial square ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu2", [10, 1000])
@pytest.mark.parametrize("k", [2, 3])
def test_bimaterial_guaranteed_upper_bound(oracle_mod, k, mu2):
    """eta^2 = sum energy + sum (sqrt(wsym) + sqrt(osc))^2, with energy and wsym divided by mu_T and the oscillation
    taken with korn / sqrt(mu_T), bounds the energy error sqrt(int mu (2 |eps(e)|^2 + pi_1 (div e)^2)) of the P_k solution
    from above on every level, and the error converges with order k: the local weights 1 / mu_T hold on this problem at
    both contrasts.  As in test_elasticity_guaranteed_upper_bound the effectivity is large because of the Korn constants
    (C_K = 11.5 ... 25.8), so no sharpness is asserted.  Measured (n = 4 / 8 / 16):
      k = 2, mu2 = 10    eta / e 19.20 / 14.46 / 11.46,  error rates 1.996, 2.014, sqrt(sum energy) / e 1.40 ... 1.41,
                         sqrt(sum wsym) / e 11.8 / 11.0 / 9.9, sqrt(sum osc) / e 7.8 / 3.7 / 1.7
      k = 3, mu2 = 10    eta / e 19.96 / 15.00 / 12.30,  error rates 2.956, 2.996, sqrt(sum energy) / e 1.41 ... 1.42
      k = 2, mu2 = 1000  eta / e 18.91 / 14.48 / 11.58,  error rates 2.025, 2.008, sqrt(sum energy) / e 1.38 ... 1.40
      k = 3, mu2 = 1000  eta / e 17.53 / 13.53 / 11.39,  error rates 2.954, 2.981, sqrt(sum energy) / e 1.31 ... 1.32
    (mu2 = 1, the jump of pi_1 alone: 19.63 / 14.43 / 11.29 at k = 2, 22.53 / 16.61 / 13.38 at k = 3.)"""
    eff, errs = [], []
    for n in (4, 8, 16):
        P = sc.problem(n, k, mu2)
        energy, wsym, osc, korn = sc.host_terms(oracle_mod, P, k)
        eta = sc.estimate(energy, wsym, osc)
        eff.append(eta / P["err"])
        errs.append(P["err"])
        print(f"k={k} mu2={mu2} n={n}: e = {P['err']:.6e}, eta / e = {eff[-1]:.3f}, sqrt(sum energy) / e = "
              f"{np.sqrt(energy.sum()) / P['err']:.4f}, sqrt(sum wsym) / e = {np.sqrt(wsym.sum()) / P['err']:.4f}, "
              f"sqrt(sum osc) / e = {np.sqrt(osc.sum()) / P['err']:.4f}, C_K in [{korn.min():.2f}, {korn.max():.2f}]")
        assert eta / P["err"] >= 1.0 - 1e-10, eff
    rates = [float(np.log2(errs[i] / errs[i + 1])) for i in range(2)]
    print(f"k={k} mu2={mu2}: error rates {rates[0]:.3f}, {rates[1]:.3f}")
    assert rates[1] > k - 0.2, rates
