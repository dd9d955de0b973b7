"""The numpy statements of tests/estimator_cases.py against themselves in long double, and the oracle's Korn constants
against a long-double restatement: the reference alone must fit into HALF of the bound before the device is given the
whole of it (tests/test_gpu_estimator_meshes.py).  No device.  The largest |float64 - long double| / bound per quantity is
printed per case; measured (k = 1 ... 4, every mesh): at most 0.12 of the bound (sig2 on disk100 at k = 1).  The oracle's
Korn constants stay within 0.28 of their tolerance (disk100)."""

import numpy as np
import pytest

import estimator_cases as E

CASES = E.CASES + [(n, k, d) for n in E.LOWDEG_MESHES_HOST for k, d in E.LOWDEG]


def test_table_keeps_its_point():
    E.check_table()
    assert np.finfo(np.longdouble).nmant >= 63, "the long-double evaluation needs more than 53 bits"


@pytest.mark.parametrize("case", CASES, ids=E.case_id)
def test_float64_statement_within_half_of_the_bound(case):
    name, k, d = case
    stress = d == k - 1
    lo, hi = E.quantities(name, k, d, np.float64, stress=stress), E.quantities(name, k, d, np.longdouble, stress=stress)
    worst = {}
    for key, (val, A, c) in lo.items():
        ref = hi[key][0]
        assert val.dtype == np.float64 and ref.dtype == np.longdouble and val.shape == ref.shape
        assert np.all(np.isfinite(val)) and np.all(np.isfinite(A))
        diff, bound = E.deviation(key, val, ref, A, c)
        worst[key] = E.ratio(diff, bound)
        assert np.all(diff <= 0.5 * bound), (key, case, worst[key])
    print(f"{E.case_id(case)}: |float64 - long double| / bound: " + " ".join(f"{q}={v:.3f}" for q, v in worst.items()))


def test_statements_agree_with_the_quadrature_statements():
    """The exact-integral statements against the quadrature statements of check_eqlb_conditions on one mesh: two
    derivations of the same quantities (1e-11: the figure the quadrature statements were given so far)."""
    from dolfinx_eqlb_amd.eqlb import check_eqlb_conditions as chk
    name, k, d = "wg256", 3, 2
    mesh, D = E.mesh_of(name), E.data(name, k, d)
    q = E.quantities(name, k, d)
    x, G, f = D["x"][0], D["G"][0], D["f"][0]

    def close(a, b):
        return np.abs(a - b).max() <= 1e-11 * np.abs(b).max()
    res, _ = chk.divergence_residual(mesh, k, x, G, f)
    assert abs(np.sqrt(q["div2"][0].sum()) - res) <= 1e-11 * res
    e_ref, w_ref = chk.stress_estimator_terms(mesh, k, D["x"][:2], D["korn"], 50.0)
    assert close(q["energy50"][0], e_ref) and close(q["wsym50"][0], w_ref)
    assert close(q["asym"][0], chk.weak_symmetry_residual(mesh, k, D["x"][:2])[1])
    span = np.abs(mesh.x[:, :2]).max()
    assert close(q["osc"][0], chk.oscillation_term(mesh, k, x, G, lambda a, b: E.f_osc(0, a / span, b / span), E.QDEG,
                                                   D["korn"]))
    ref = np.array([chk.boundary_flux_residual(mesh, k, x, G, [fc], boundary_values=D["bv"][0]) for fc in D["facets"]])
    assert close(np.abs(q["bres_bv"][0]).max(axis=1), ref)
    from test_gpu_estimate_lower_degree import ev_flux_error2, jump_moments
    assert close(np.abs(q["jump"][0]).max(axis=1), jump_moments(mesh, k, d, x, G))
    assert close(q["sig2_ev"][0], ev_flux_error2(mesh, k, d, x, G))


@pytest.mark.parametrize("layout", E.KORN_LAYOUTS)
@pytest.mark.parametrize("name", E.KORN_MESHES)
def test_oracle_korn_against_long_double(oracle_mod, name, layout):
    mesh = E.mesh_of(name)
    ref, per_node, cks, amp, tol = E.korn_reference(oracle_mod, name, layout)
    diff = np.abs(ref - E.korn_cells(mesh, cks)).astype(np.float64)
    r = E.ratio(diff, tol)
    print(f"{name} {layout}: c_K^2 in [{ref.min():.3e}, {ref.max():.3e}], largest relative tolerance "
          f"{(tol / ref).max():.3e}, largest amp {amp.max():.3e}, |oracle - long double| / tolerance = {r:.3f}")
    assert np.all(diff <= 0.5 * tol)
    if name == "aspect1000":
        assert 1e7 < ref.max() < 1e9 and np.median(ref) > 1e7
