"""The P_p Poisson and elasticity operators as CSR on the device (cpp.PrimalPoisson.matrix, cpp.PrimalElasticity.matrix,
cpp.csr_apply; eqlb_primal_matrix_*, eqlb_elasticity_matrix_*, eqlb_csr_apply) against the numpy statement of
lsolver.primal (matrix, csr_apply): indptr, indices and values bit for bit, term by term, in host and device memory
space; the raw diagonal against the handle's own; the refill after a change of the handle; the product; two calls and a
caller's stream; the handle before and after the pattern; the refusals; and a sparse direct solve of the assembled
matrix against the device's own CG.

  triangle, right1            one and two cells, no shared interior row
  bowtie, two_parts, hole     a pinched vertex, two components, two boundary loops
  disk100 at p = 4            a hub row of more than a thousand entries
  wg128, wg256                whole workgroups of cells
  sq91                        more pairs and more rows than one pass of the grid-stride kernels
  aspect1000, tiny_far        geometry
The cases and the counts of roundings are those of tests/matrix_cases.py."""

import numpy as np
import pytest

import matrix_cases as mx
import primal_mesh_cases as pm
from primal_cases import U, ratio

pytestmark = pytest.mark.gpu

SMALL = ("triangle", "right1", "bowtie", "two_parts", "hole", "wg128", "wg256", "aspect1000", "tiny_far")
_CACHE = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def device_mesh(name):
    if name not in _CACHE:
        from dolfinx_eqlb_amd import cpp
        _CACHE[name] = cpp.DeviceMesh(pm.mesh_of(name))
    return _CACHE[name]


def layout_of(problem, name):
    return "inner" if (problem, name) == ("poisson", "hole") else "all"


def pair(problem, name, p, variant):
    """(statement, handle) of one case with the same terms and mask"""
    from dolfinx_eqlb_amd import cpp
    op, k, args = mx.statement(problem, pm.mesh_of(name), p, variant, layout_of(problem, name))
    h = mx.device_handle(cpp, device_mesh(name), problem, p, k, args)
    assert h.ndofs == op.ndofs
    return op, h, k


def to_host(t):
    return t.cpu().numpy()


def check_arrays(op, h, device):
    """the three arrays, raw and eliminated, against the statement; the raw diagonal against the handle's own"""
    import scipy.sparse as sp
    for eliminate in (False, True):
        ip, ix, v = op.matrix(eliminate)
        for call in range(2):        # a second call gives the same bits
            got = h.matrix(eliminate, device=device)
            gp, gx, gv = [to_host(t) for t in got] if device else got
            assert gp.dtype == np.int64 and gx.dtype == np.int32
            assert np.array_equal(gp, ip) and np.array_equal(gx, ix)
            assert np.array_equal(bits(gv), bits(v))
        if not eliminate:
            n = ip.size - 1
            assert np.array_equal(bits(sp.csr_matrix((gv, gx, gp), shape=(n, n)).diagonal()), bits(h.diagonal()))
    return ip


@pytest.mark.parametrize("problem", ["poisson", "elasticity"])
@pytest.mark.parametrize("name", SMALL)
def test_arrays_have_the_bits_of_the_statement(name, problem):
    """p = 1 ... 4, eliminate 0 and 1, each term alone and all together, host and device memory space"""
    for p in (1, 2, 3, 4):
        for variant in mx.VARIANTS[problem]:
            op, h, _ = pair(problem, name, p, variant)
            check_arrays(op, h, device=False)
            check_arrays(op, h, device=True)
            h.close()


@pytest.mark.parametrize("problem", ["poisson", "elasticity"])
def test_a_hub_row_of_more_than_a_thousand_entries(problem):
    """disk100 at p = 4: the row of the hub has 1001 pairs (101 vertices, 600 facet and 300 interior DOFs)"""
    for variant in ("none", "all"):
        op, h, _ = pair(problem, "disk100", 4, variant)
        ip = check_arrays(op, h, device=False)
        assert np.diff(ip).max() == 1001 * (1 if problem == "poisson" else 2)
        h.close()


@pytest.mark.parametrize("problem,p", [("poisson", 3), ("elasticity", 2)])
def test_more_than_one_pass_of_the_grid_stride_kernels(problem, p):
    """sq91: more pairs than one pass of the fill and export kernels, more rows than one pass of the product"""
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.lsolver import primal
    op, h, _ = pair(problem, "sq91", p, "all")
    ip, ix, v = op.matrix()
    bs = 1 if problem == "poisson" else 2
    assert ix.size // (bs * bs) > mx.PAIRS_PER_PASS and ip.size - 1 > mx.ROWS_PER_PASS
    gp, gx, gv = h.matrix()
    assert np.array_equal(gp, ip) and np.array_equal(gx, ix) and np.array_equal(bits(gv), bits(v))
    assert np.array_equal(bits(h.matrix_values(True)), bits(op.matrix(True)[2]))
    x = np.random.default_rng(p).standard_normal(ip.size - 1)
    assert np.array_equal(bits(cpp.csr_apply(ip, ix, v, x)), bits(primal.csr_apply(ip, ix, v, x)))
    h.close()


@pytest.mark.parametrize("problem", ["poisson", "elasticity"])
def test_values_follow_the_handle_on_the_same_pattern(problem):
    """matrix_values after set_reaction, set_shear / set_diffusion, set_dirichlet and back: the values are those of the
    statement with the same terms, the pattern arrays are untouched, switching a term off restores the first bits"""
    name, p = "hole", 2
    mesh = pm.mesh_of(name)
    op, h, _ = pair(problem, name, p, "none")
    ip, ix, first = h.matrix()
    assert np.array_equal(bits(first), bits(op.matrix()[2]))
    full = mx.coefficients(problem, mesh, "all")

    def same(eliminate=False):
        assert np.array_equal(bits(h.matrix_values(eliminate)), bits(op.matrix(eliminate)[2]))
        gp, gx, _ = h.matrix(eliminate)
        assert np.array_equal(gp, ip) and np.array_equal(gx, ix)

    for who in (op, h):
        who.set_reaction(cell_c=full["c"])
    same()
    for who in (op, h):
        who.set_reaction(2.5)
    same()
    if problem == "poisson":
        for who in (op, h):
            who.set_diffusion(full["D"])
        same()
        for who in (op, h):
            who.set_diffusion(None)
    else:
        for who in (op, h):
            who.set_shear(cell_mu=full["mu"])
        same()
        for who in (op, h):
            who.set_shear(0.5)
        same()
        for who in (op, h):
            who.set_shear(1.0)
    same()
    for who in (op, h):
        who.set_reaction(0.0)
    assert np.array_equal(bits(h.matrix_values()), bits(first))
    # another mask: the eliminated values follow it, the raw ones do not see it
    args = (pm.dirichlet_facets(mesh, "part"),) * (1 if problem == "poisson" else 2)
    for who in (op, h):
        who.set_dirichlet(*args)
    same(True)
    assert np.array_equal(bits(h.matrix_values()), bits(first))
    h.close()


@pytest.mark.parametrize("problem", ["poisson", "elasticity"])
@pytest.mark.parametrize("name,ps", [("bowtie", (1, 2, 3, 4)), ("disk100", (4,))])
def test_product_equals_the_statement_and_the_matrix_free_apply(name, ps, problem):
    """cpp.csr_apply has the bits of lsolver.primal.csr_apply, from host arrays and from device tensors, and lies within
    c 2^-53 A of the device's matrix-free apply: A the statement on absolute values, c = matrix_cases.chain"""
    import torch
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.lsolver import primal
    worst = 0.0
    for p in ps:
        op, h, k = pair(problem, name, p, "all")
        ip, ix, v = h.matrix()
        x = np.random.default_rng(pm.seed_of("gpu-matrix", problem, name, p)).standard_normal(ip.size - 1)
        ref = primal.csr_apply(ip, ix, v, x)
        for call in range(2):
            assert np.array_equal(bits(cpp.csr_apply(ip, ix, v, x)), bits(ref))
        dev = [torch.from_numpy(a).cuda() for a in (ip, ix, v, x)]
        assert np.array_equal(bits(to_host(cpp.csr_apply(*dev))), bits(ref))
        y = h.apply(x)
        yabs = op.apply(x, return_abs=True)[1]
        c = mx.chain(problem, p, pm.valence(pm.mesh_of(name)), int(np.diff(ip).max()), k)
        diff, bound = np.abs(ref - y), c * U * yabs
        assert np.all(diff <= bound)
        worst = max(worst, ratio(diff, bound))
        h.close()
    print(f"{name} {problem}: largest share of the bound of the product = {worst:.4f}")


@pytest.mark.parametrize("problem", ["poisson", "elasticity"])
def test_a_callers_non_blocking_stream(problem):
    """the same bits from a caller's stream, pattern build included"""
    import torch
    op, h, _ = pair(problem, "wg256", 3, "all")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        got = [h.matrix(e, device=True, stream=st.cuda_stream) for e in (False, True, False)]
        vals = h.matrix_values(True, device=True, stream=st.cuda_stream)
    st.synchronize()
    for e, g in zip((False, True, False), got):
        ip, ix, v = op.matrix(e)
        assert np.array_equal(to_host(g[0]), ip) and np.array_equal(to_host(g[1]), ix)
        assert np.array_equal(bits(to_host(g[2])), bits(v))
    assert np.array_equal(bits(to_host(vals)), bits(op.matrix(True)[2]))
    h.close()


@pytest.mark.parametrize("problem", ["poisson", "elasticity"])
def test_the_handle_is_the_same_before_and_after_the_pattern(problem):
    """apply, diagonal and solve give the same bits before the pattern was built, with it, and after its release; a
    released pattern is built again"""
    op, h, _ = pair(problem, "bowtie", 2, "all")
    b, u0, start = pm.solve_data(op, problem, "bowtie", 2, inhomogeneous=True)

    def state():
        u, info = h.solve(b, start, rtol=1e-10, maxit=5000)
        return [bits(h.apply(start)), bits(h.apply(start, masked=True)), bits(h.diagonal()), bits(u),
                np.array([info["iterations"], info["converged"]])]

    before = state()
    m1 = h.matrix(True)
    for a, c in zip(before, state()):
        assert np.array_equal(a, c)
    h.matrix_release()
    for a, c in zip(before, state()):
        assert np.array_equal(a, c)
    m2 = h.matrix(True)
    assert all(np.array_equal(a, c) for a, c in zip(m1[:2], m2[:2])) and np.array_equal(bits(m1[2]), bits(m2[2]))
    h.matrix_release()
    h.matrix_release()      # (nothing to free: no error)
    h.close()


@pytest.mark.parametrize("problem", ["poisson", "elasticity"])
def test_refusals_by_name_and_the_next_call_works(problem):
    from dolfinx_eqlb_amd import cpp
    L = cpp.lib()
    op, h, _ = pair(problem, "right1", 2, "all")
    pre = "eqlb_primal_matrix_" if problem == "poisson" else "eqlb_elasticity_matrix_"
    n = (1 if problem == "poisson" else 2) * h.ndofs

    def refused(call, who, what):
        with pytest.raises(RuntimeError, match=who + ".*" + what):
            call()

    def status(code, who, what):
        assert code == -1
        msg = L.eqlb_last_error().decode()
        assert msg.startswith(who) and what in msg, msg

    big = np.zeros(4096)
    ipb, ixb = np.zeros(n + 1, dtype=np.int64), np.zeros(4096, dtype=np.int32)
    host = cpp.MEM_HOST
    # before the pattern
    refused(lambda: h.matrix_export_raw(ipb.ctypes.data, ixb.ctypes.data, host), pre + "export", "no pattern")
    refused(lambda: h.matrix_values_raw(0, big.ctypes.data, big.size, host), pre + "values", "no pattern")
    status(getattr(L, pre + "pattern")(h._h, None, None), pre + "pattern", "null")
    nnz = h.matrix_pattern_raw()
    assert nnz == op.matrix()[1].size and nnz <= big.size
    # null arguments, capacity, eliminate, memory space
    refused(lambda: h.matrix_export_raw(None, ixb.ctypes.data, host), pre + "export", "null")
    refused(lambda: h.matrix_export_raw(ipb.ctypes.data, None, host), pre + "export", "null")
    refused(lambda: h.matrix_values_raw(0, None, nnz, host), pre + "values", "null")
    refused(lambda: h.matrix_values_raw(0, big.ctypes.data, nnz - 1, host), pre + "values", "capacity")
    refused(lambda: h.matrix_values_raw(2, big.ctypes.data, nnz, host), pre + "values", "eliminate = 2")
    refused(lambda: h.matrix_values_raw(-1, big.ctypes.data, nnz, host), pre + "values", "eliminate = -1")
    refused(lambda: h.matrix_values(eliminate=0.5), pre + "values", "eliminate")
    refused(lambda: h.matrix_values_raw(0, big.ctypes.data, nnz, 7), pre + "values", "memory space")
    refused(lambda: h.matrix_export_raw(ipb.ctypes.data, ixb.ctypes.data, 7), pre + "export", "memory space")
    assert np.all(big == 0.0) and np.all(ipb == 0) and np.all(ixb == 0)        # nothing was written
    ip, ix, v = op.matrix(True)
    x = np.ones(n)
    refused(lambda: cpp.csr_apply_raw(2 ** 31, ip.ctypes.data, ix.ctypes.data, v.ctypes.data, x.ctypes.data,
                                      x.ctypes.data, host), "eqlb_csr_apply", "n = 2147483648")
    refused(lambda: cpp.csr_apply_raw(n, ip.ctypes.data, None, v.ctypes.data, x.ctypes.data, x.ctypes.data, host),
            "eqlb_csr_apply", "null")
    refused(lambda: cpp.csr_apply_raw(n, ip.ctypes.data, ix.ctypes.data, v.ctypes.data, x.ctypes.data, x.ctypes.data,
                                      7), "eqlb_csr_apply", "memory space")
    # the next valid calls work
    gp, gx, gv = h.matrix(True)
    assert np.array_equal(gp, ip) and np.array_equal(gx, ix) and np.array_equal(bits(gv), bits(v))
    from dolfinx_eqlb_amd.lsolver import primal
    assert np.array_equal(bits(cpp.csr_apply(ip, ix, v, x)), bits(primal.csr_apply(ip, ix, v, x)))
    h.close()


# ---- end to end: a sparse direct solve of the assembled matrix against the device's own CG ----------------------------------
def check_direct_solve(problem, name, p, op, h, k, b, u_d, rtol=1e-10):
    """spsolve on the device-assembled eliminated matrix with the lifted right-hand side residual(b, u_D): the relative
    residual of u = u_D + w through the device residual is below 1e-8; and the energy-norm distance to the device's
    solve(rtol) is below what that rtol allows:
        A_ff e = r_direct - r_cg on the free rows, so || e ||_A^2 = (A e)^T A_ff^-1 (A e) <= || A e ||^2 / lambda_min and
        || e ||_A <= (tol + || r_direct || + delta) / sqrt(lambda_min(A_ff))
    with tol = rtol nb >= || r_cg || (info["tol"]), || r_direct || the device's residual norm of the direct solution,
    lambda_min of the assembled matrix on the free rows (computed here), and delta = 2 c 2^-53 || |A| |u| ||_2 for the
    two residuals being formed by the matrix-free product and e being measured with the assembled one
    (c = matrix_cases.chain)."""
    import scipy.sparse.linalg as spla
    from dolfinx_eqlb_amd.lsolver import primal
    ip, ix, ve = h.matrix(eliminate=True)
    assert np.array_equal(bits(ve), bits(op.matrix(True)[2]))
    w = spla.spsolve(mx.to_scipy((ip, ix, ve)).tocsc(), h.residual(b, u_d))
    u = u_d + w
    _, rn, nb = h.residual(b, u, norms=True)
    print(f"{problem} {name} p={p}: relative residual of the direct solve {rn / nb:.2e}")
    assert rn / nb < 1e-8
    ucg, info = h.solve(b, u_d, rtol=rtol, maxit=20000)
    assert info["converged"] == 1
    free = np.nonzero(~op.fixed)[0]
    Aff = mx.to_scipy((ip, ix, ve))[free][:, free]
    lam = np.linalg.eigvalsh(Aff.toarray())[0]
    assert lam > 0.0
    e = (ucg - u)[free]
    err = np.sqrt(e @ (Aff @ e))
    c = mx.chain(problem, p, pm.valence(pm.mesh_of(name)), int(np.diff(ip).max()), k)
    raw = h.matrix_values()
    delta = 2.0 * c * U * np.linalg.norm(primal.csr_apply(ip, ix, np.abs(raw), np.abs(ucg)))
    bound = (info["tol"] + rn + delta) / np.sqrt(lam)
    print(f"  energy distance to solve(rtol={rtol:g}) {err:.3e}, bound {bound:.3e} (lambda_min {lam:.3e}, tol "
          f"{info['tol']:.3e}, delta {delta:.3e})")
    assert err <= bound


def test_direct_solve_poisson_with_kappa_and_reaction_on_hole():
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.lsolver import primal
    name, p = "hole", 2
    mesh = pm.mesh_of(name)
    k = dict(coeff=mx.pc.kappa_of(mesh.ncells), D=None, mu=None, c=mx.rc.c_of(mesh.ncells))
    args = (pm.dirichlet_facets(mesh, "inner"),)
    op = primal.PoissonOperator(mesh, p, k["coeff"])
    op.set_reaction(cell_c=k["c"])
    op.set_dirichlet(*args)
    h = mx.device_handle(cpp, device_mesh(name), "poisson", p, k, args)
    data = pm.vectors("poisson", mesh, p, op.ndofs, name)
    b = h.load(data["d"], data["f"], data["e"])
    u_d = np.where(op.fixed, data["u"], 0.0)
    check_direct_solve("poisson", name, p, op, h, k, b, u_d)
    h.close()


def test_direct_solve_cook_like_elasticity():
    """clamped on the left part of the boundary, tractions on the rest (traction_load), P_2, pi_1 cell-wise"""
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.eqlb.bcs import fluxbc
    from dolfinx_eqlb_amd.lsolver import primal
    name, p = "delaunay", 2
    mesh = pm.mesh_of(name)
    k = dict(coeff=mx.ec.pi1_of(mesh.ncells), D=None, mu=None, c=None)
    clamped = pm.dirichlet_facets(mesh, "part")
    loaded = np.setdiff1d(mesh.boundary_facets(), clamped)
    assert clamped.size > 0 and loaded.size > 0
    args = (clamped, clamped)
    op = primal.ElasticityOperator(mesh, p, mx.PI_SCALAR, k["coeff"])
    op.set_dirichlet(*args)
    h = mx.device_handle(cpp, device_mesh(name), "elasticity", p, k, args)
    g = [lambda x, y: 0.0 * x, lambda x, y: -1.0 + 0.0 * x]          # a shear load, as on Cook's membrane
    be = primal.traction_load(mesh, p, [[fluxbc(g[r], loaded, scalar=True)] for r in range(2)])
    data = pm.vectors("elasticity", mesh, p, 2 * op.ndofs, name)
    b = h.load(data["d"], 0.0 * data["f"], be)
    check_direct_solve("elasticity", name, p, op, h, k, b, np.zeros(2 * op.ndofs))
    h.close()
