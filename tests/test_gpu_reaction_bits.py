"""The reaction term of the P_p solves on the device (eqlb_primal_set_reaction / eqlb_elasticity_set_reaction) against
the numpy statement (lsolver.primal: set_reaction), bit for bit, on the meshes of tests/primal_mesh_cases.py: apply
(masked and raw), diagonal and residual with both norms, with a scalar c, a cell-wise c with zeros, in host and in
device memory; the load is unchanged.  Then several columns (apply_many / solve_many are the single calls), switching
the term on, off and over, and the refusals.  Every handle here is made for its test: a reaction left on a shared one
would change the tests of other files."""

import numpy as np
import pytest

import primal_mesh_cases as pm
import reaction_cases as rc
from test_gpu_primal_many import compare, same_info
from test_gpu_primal_meshes import device_mesh, make_handle
from test_gpu_primal_solve import bits

pytestmark = pytest.mark.gpu

U = rc.U
RTOL = 1e-10


def case(problem, name, p):
    """the statement, a handle of its own and the vectors of one (problem, mesh, p), Dirichlet all around"""
    mesh = pm.mesh_of(name)
    op, coeff, args = pm.statement(problem, mesh, p, "all")
    h = make_handle(problem, device_mesh(name), p, coeff, args)
    assert h.ndofs == op.ndofs
    n = op.fixed.size
    c = dict(op=op, h=h, n=n, mesh=mesh, coeff=coeff, args=args, **pm.vectors(problem, mesh, p, n, name))
    c["b"] = op.load(c["d"], c["f"], c["e"])     # (the load knows no reaction term)
    c["plain"] = op.apply(c["u"])
    return c


def statement_values(c):
    op, u, b = c["op"], c["u"], c["b"]
    return dict(y=op.apply(u), ym=op.apply(u, masked=True), dg=op.diagonal(), rs=op.residual(b, u),
                nbs=op.reference_norm(b, u))


def check_host(c, calls=2):
    h, u, b, n = c["h"], c["u"], c["b"], c["n"]
    s = statement_values(c)
    for call in range(calls):   # a second call gives the same bits
        assert np.array_equal(bits(h.apply(u)), bits(s["y"]))
        assert np.array_equal(bits(h.apply(u, masked=True)), bits(s["ym"]))
        assert np.array_equal(bits(h.diagonal()), bits(s["dg"]))
        r, rn, nb = h.residual(b, u, norms=True)
        assert np.array_equal(bits(r), bits(s["rs"]))
        # the norms are sums in another order: n roundings
        assert abs(rn - np.sqrt(np.sum(s["rs"] * s["rs"]))) <= n * U * rn
        assert abs(nb - s["nbs"]) <= n * U * nb
        assert np.array_equal(bits(h.load(c["d"], c["f"], c["e"])), bits(b))      # unchanged
    return s


def check_device(c, cell_c):
    """the coefficient, the vectors and the results in device memory"""
    import torch
    h, b, n = c["h"], c["b"], c["n"]
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    u, bb, f, e, cc = t(c["u"]), t(b), t(c["f"]), t(c["e"]), t(cell_c)
    out = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    norms = torch.full((2,), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    h.set_reaction_raw(0.0, cc.data_ptr())
    s = statement_values(c)
    for call in range(2):
        h.apply_raw(u.data_ptr(), out.data_ptr(), False)
        assert np.array_equal(bits(out.cpu().numpy()), bits(s["y"]))
        h.apply_raw(u.data_ptr(), out.data_ptr(), True)
        assert np.array_equal(bits(out.cpu().numpy()), bits(s["ym"]))
        h.diagonal_raw(out.data_ptr())
        assert np.array_equal(bits(out.cpu().numpy()), bits(s["dg"]))
        h.residual_raw(bb.data_ptr(), u.data_ptr(), out.data_ptr(), norms.data_ptr())
        assert np.array_equal(bits(out.cpu().numpy()), bits(s["rs"]))
        nv = norms.cpu().numpy()
        assert abs(nv[0] - np.sqrt(np.sum(s["rs"] * s["rs"]))) <= n * U * nv[0]
        assert abs(nv[1] - s["nbs"]) <= n * U * nv[1]
        h.load_raw(c["d"], f.data_ptr(), e.data_ptr(), out.data_ptr())
        assert np.array_equal(bits(out.cpu().numpy()), bits(b))
    assert np.array_equal(bits(cc.cpu().numpy()), bits(cell_c))   # the input is not touched
    cc.fill_(float("nan"))                                        # ... and was copied: the handle does not read it again
    torch.cuda.synchronize()
    h.apply_raw(u.data_ptr(), out.data_ptr(), False)
    assert np.array_equal(bits(out.cpu().numpy()), bits(s["y"]))


# ---- 1. bit for bit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem", ["poisson", "elasticity"])
@pytest.mark.parametrize("name", rc.BIT_MESHES)
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_reaction_bit_for_bit(problem, name, p):
    c = case(problem, name, p)
    op, h, ncells = c["op"], c["h"], c["mesh"].ncells
    # a scalar
    op.set_reaction(3.75)
    h.set_reaction(3.75)
    s = check_host(c)
    assert not np.array_equal(s["y"], c["plain"])
    # cell-wise, with zeros, host memory: replaces the scalar
    cc = rc.c_of(ncells)
    op.set_reaction(cell_c=cc)
    h.set_reaction(cell_c=cc)
    check_host(c)
    # cell-wise, device memory: replaces the array
    cc2 = rc.c_of(ncells, seed=5)
    cc2[-1] = 2.0 ** -3
    op.set_reaction(cell_c=cc2)
    check_device(c, cc2)


@pytest.mark.parametrize("problem,p", [("poisson", 3), ("elasticity", 2)])
def test_reaction_on_more_than_one_pass(problem, p):
    c = case(problem, "sq91", p)
    assert c["n"] > pm.ROWS_PER_PASS
    cc = rc.c_of(c["mesh"].ncells)
    c["op"].set_reaction(cell_c=cc)
    c["h"].set_reaction(cell_c=cc)
    s = check_host(c, calls=1)
    assert not np.array_equal(s["y"], c["plain"])


# ---- 2. several columns --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wg256", "disk100"])
@pytest.mark.parametrize("p", [1, 4])
@pytest.mark.parametrize("nrhs", [2, 3, 4, 5])
def test_columns_with_a_reaction_term_are_the_single_calls(name, p, nrhs):
    c = case("poisson", name, p)
    op, h, n = c["op"], c["h"], c["n"]
    cc = rc.c_of(c["mesh"].ncells)
    op.set_reaction(cell_c=cc)
    h.set_reaction(cell_c=cc)
    rng = np.random.default_rng(pm.seed_of("reaction-columns", name, p, nrhs))
    V = rng.standard_normal((nrhs, n))
    for masked in (False, True):
        ref = np.stack([h.apply(V[k], masked=masked) for k in range(nrhs)])
        assert np.array_equal(bits(ref[0]), bits(op.apply(V[0], masked=masked)))
        assert np.array_equal(bits(h.apply_many(V, masked=masked)), bits(ref)), masked
    B = np.where(op.fixed, 0.0, rng.standard_normal((nrhs, n)))
    B[1] *= 1e-3
    U0 = np.where(op.fixed, rng.standard_normal((nrhs, n)), 0.0)
    infos = compare(h.solve_many, h.solve, B, U0, rtol=RTOL, maxit=5000)
    assert all(i["converged"] == 1 and i["breakdown"] == 0 for i in infos)
    # a NaN column leaves the others alone
    X, _ = h.solve_many(B, U0, rtol=RTOL, maxit=5000)
    Bn = B.copy()
    Bn[1, np.nonzero(~op.fixed)[0][7]] = np.nan
    Xn, infos_n = h.solve_many(Bn, U0, rtol=RTOL, maxit=5000)
    assert infos_n[1]["breakdown"] == 1 and infos_n[1]["converged"] == 0
    for k in range(nrhs):
        if k != 1:
            assert np.array_equal(bits(Xn[k]), bits(X[k])) and same_info(infos_n[k], infos[k]), k


# ---- 3. switching ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem", ["poisson", "elasticity"])
@pytest.mark.parametrize("p", [1, 4])
def test_switching_and_refusals(problem, p):
    c = case(problem, "wg256", p)
    op, h, u, ncells = c["op"], c["h"], c["u"], c["mesh"].ncells
    fresh = make_handle(problem, device_mesh("wg256"), p, c["coeff"], c["args"])
    y0, d0 = fresh.apply(u), fresh.diagonal()
    assert np.array_equal(bits(y0), bits(c["plain"]))
    h.set_reaction(2.5)
    assert not np.array_equal(h.apply(u), y0) and np.all(h.diagonal() > d0)
    h.set_reaction(0.0)                      # off: the handle is as created
    assert np.array_equal(bits(h.apply(u)), bits(y0)) and np.array_equal(bits(h.diagonal()), bits(d0))
    h.set_reaction(cell_c=rc.c_of(ncells))
    h.set_reaction(7.0)                      # a repeated call replaces the coefficient: the scalar, not the array
    op.set_reaction(7.0)
    y7, d7 = op.apply(u), op.diagonal()
    assert np.array_equal(bits(h.apply(u)), bits(y7)) and np.array_equal(bits(h.diagonal()), bits(d7))
    # refusals (host memory) name the cell and leave the handle as it was
    who = "eqlb_primal_set_reaction" if problem == "poisson" else "eqlb_elasticity_set_reaction"
    for value, where in ((-1.0, 5), (float("nan"), 0), (float("inf"), ncells - 1)):
        bad = np.ones(ncells)
        bad[where] = value
        with pytest.raises(RuntimeError, match=who + r": cell_c\[%d\] = " % where):
            h.set_reaction(cell_c=bad)
        assert np.array_equal(bits(h.apply(u)), bits(y7)) and np.array_equal(bits(h.diagonal()), bits(d7))
    for value in (-2.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match=who + ": c = "):
            h.set_reaction(value)
    with pytest.raises(RuntimeError, match="Input sizes does not match"):
        h.set_reaction(cell_c=np.ones(ncells + 1))
    assert np.array_equal(bits(h.apply(u)), bits(y7)) and np.array_equal(bits(h.diagonal()), bits(d7))
    h.set_reaction()                         # the defaults switch the term off
    assert np.array_equal(bits(h.apply(u)), bits(y0)) and np.array_equal(bits(h.diagonal()), bits(d0))


@pytest.mark.parametrize("problem", ["poisson", "elasticity"])
def test_pybind_module_sets_the_reaction(problem):
    """_cpp.PrimalPoisson / _cpp.PrimalElasticity.set_reaction: the same bits as the statement"""
    from dolfinx_eqlb_amd.eqlb import _adapter
    cm = _adapter.module()
    c = case(problem, "wg128", 2)
    op, u, mesh = c["op"], c["u"], c["mesh"]
    m = _adapter.cpp_mesh(mesh)
    h = cm.PrimalPoisson(m, 2, c["coeff"]) if problem == "poisson" else cm.PrimalElasticity(m, 2, 1.0, c["coeff"])
    h.set_dirichlet(*c["args"])
    cc = rc.c_of(mesh.ncells)
    for kw in (dict(c=0.5), dict(cell_c=cc), dict()):
        op.set_reaction(**kw)
        h.set_reaction(**kw)
        assert np.array_equal(bits(h.apply(u, True)), bits(op.apply(u, masked=True)))
        assert np.array_equal(bits(h.diagonal()), bits(op.diagonal()))
