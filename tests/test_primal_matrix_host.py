"""The assembled matrix of the P_p Poisson and elasticity operators as the numpy statement has it (lsolver.primal:
PoissonOperator.matrix, ElasticityOperator.matrix, csr_apply): against the independent quadrature assembly entry by
entry, the pattern against sets, the diagonal, the symmetry, the product against the matrix-free statement, the
eliminated matrix and a sparse direct solve with it; and the entries in header, library and bindings.  The counts of
roundings are those of tests/matrix_cases.py."""

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import matrix_cases as mx
import primal_mesh_cases as pm
from primal_cases import U, ratio

SMALL = ("triangle", "right1", "bowtie", "two_parts", "disk100")


@pytest.mark.parametrize("p", [1, 2, 3, 4])
@pytest.mark.parametrize("problem", ["poisson", "elasticity"])
@pytest.mark.parametrize("name", mx.HOST_MESHES)
def test_statement_equals_the_quadrature_assembly_entry_by_entry(name, problem, p):
    """|stmt - asm| <= 2^-53 (ts |stmt|-sum + ta |asm|-sum) for every entry of the pattern, and nothing of the assembly
    lies outside the pattern; ts, ta: matrix_cases.entry_terms with the valence of the mesh; the |asm|-sum is
    matrix_cases.assembled_abs (the head of that file says why).  With and without each term (matrix_cases.VARIANTS)."""
    from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
    mesh = pm.mesh_of(name)
    nq = make_quadrature_triangle(2 * p + 4)[1].size
    for variant in mx.VARIANTS[problem]:
        op, k, _ = mx.statement(problem, mesh, p, variant)
        A, Aabs, nvalues = mx.assembled(problem, mesh, p, k)
        ts, ta = mx.entry_terms(problem, p, pm.valence(mesh), nq, k, nvalues)
        ip, ix, v, vabs = op.matrix(return_abs=True)
        rows = np.repeat(np.arange(ip.size - 1), np.diff(ip))
        asm = np.asarray(A[rows, ix]).ravel()
        Afull = mx.assembled_abs(problem, mesh, p, k)
        assert (Afull - Aabs).min() >= -4.0 * U * Afull.max()      # it dominates the |A| of the case modules
        asm_abs = np.asarray(Afull[rows, ix]).ravel()
        diff, bound = np.abs(v - asm), U * (ts * vabs + ta * asm_abs)
        print(f"{name} {problem} p={p} {variant}: max |diff| / bound = {ratio(diff, bound):.3f} (terms {(ts, ta)})")
        assert np.all(diff <= bound)
        # the assembly has no entry outside the pattern
        S = mx.to_scipy((ip, ix, np.ones(ix.size)))
        assert (abs(A) - abs(A).multiply(S)).count_nonzero() == 0


@pytest.mark.parametrize("p", [1, 2, 3, 4])
@pytest.mark.parametrize("problem", ["poisson", "elasticity"])
@pytest.mark.parametrize("name", SMALL + ("hole",))
def test_pattern_equals_the_sets_of_the_cells(name, problem, p):
    """columns ascending, each once, the row sets those built from cell_dofs with Python sets; the pattern does not
    depend on the terms or the mask"""
    mesh = pm.mesh_of(name)
    op = mx.statement(problem, mesh, p, "none")[0]
    bs = 1 if problem == "poisson" else 2
    ip, ix, _ = op.matrix()
    sets = mx.naive_row_sets(op.cell_dofs, op.ndofs, bs)
    assert ip.dtype == np.int64 and ix.dtype == np.int32 and ip.size == bs * op.ndofs + 1 and ip[0] == 0
    for row, cols in enumerate(sets):
        got = ix[ip[row]:ip[row + 1]]
        assert np.all(np.diff(got) > 0) and set(got.tolist()) == cols, row
    other = mx.statement(problem, mesh, p, "all", "all")[0]
    for eliminate in (False, True):
        jp, jx, _ = other.matrix(eliminate)
        assert np.array_equal(jp, ip) and np.array_equal(jx, ix)


@pytest.mark.parametrize("p", [1, 2, 3, 4])
@pytest.mark.parametrize("problem", ["poisson", "elasticity"])
@pytest.mark.parametrize("name", SMALL)
def test_diagonal_symmetry_and_product(name, problem, p):
    """The raw diagonal has the bits of diagonal().  Poisson: (i, j) and (j, i) have the same bits (symmetric tables; two
    distinct DOFs share at most two cells, and a sum of two is commutative); elasticity: symmetric within the bound of
    the product (the two orders associate D_ab differently).  csr_apply(matrix, x) against apply(x):
    |difference| <= c 2^-53 A with A the statement on absolute values and c = matrix_cases.chain."""
    mesh = pm.mesh_of(name)
    worst = 0.0
    for variant in mx.VARIANTS[problem]:
        op, k, _ = mx.statement(problem, mesh, p, variant)
        from dolfinx_eqlb_amd.lsolver import primal
        ip, ix, v, vabs = op.matrix(return_abs=True)
        A = mx.to_scipy((ip, ix, v))
        assert np.array_equal(A.diagonal(), op.diagonal())
        # symmetry
        rows = np.repeat(np.arange(ip.size - 1), np.diff(ip))
        vt = np.asarray(A[ix, rows]).ravel()
        if problem == "poisson":
            assert np.array_equal(v, vt)
        else:
            Aabs = mx.to_scipy((ip, ix, vabs))
            cs = mx.entry_terms(problem, p, pm.valence(mesh), 0, k)[0]
            assert np.all(np.abs(v - vt) <= U * cs * (vabs + np.asarray(Aabs[ix, rows]).ravel()))
        # product
        x = np.random.default_rng(pm.seed_of("matrix", problem, name, p, variant)).standard_normal(ip.size - 1)
        y, yabs = op.apply(x, return_abs=True)
        c = mx.chain(problem, p, pm.valence(mesh), int(np.diff(ip).max()), k)
        diff, bound = np.abs(primal.csr_apply(ip, ix, v, x) - y), c * U * yabs
        assert np.all(diff <= bound)
        worst = max(worst, ratio(diff, bound))
    print(f"{name} {problem} p={p}: largest share of the bound of the product = {worst:.4f}")


@pytest.mark.parametrize("p", [1, 2, 3, 4])
@pytest.mark.parametrize("problem,name,layout", [("poisson", "hole", "inner"), ("poisson", "two_parts", "all"),
                                                 ("poisson", "disk100", "part"), ("elasticity", "bowtie", "all"),
                                                 ("elasticity", "delaunay", "mixed")])
def test_eliminated_matrix_and_direct_solve(problem, name, layout, p):
    """eliminate=True is P A P + (I - P) formed from the raw matrix, entry by entry.  spsolve of it with the lifted
    right-hand side residual(b, u_D) gives u = u_D + w whose residual through the statement, relative to the reference
    norm of pcg, is below the 1e-8 that solve stops at (a condition, not a measurement: a direct solve sits near
    1e-14)."""
    import scipy.sparse.linalg as spla
    mesh = pm.mesh_of(name)
    op = mx.statement(problem, mesh, p, "all", layout)[0]
    ip, ix, v = op.matrix()
    jp, jx, ve = op.matrix(eliminate=True)
    assert np.array_equal(ip, jp) and np.array_equal(ix, jx)
    assert np.array_equal(ve, mx.eliminated_from_raw(ip, ix, v, op.fixed))
    b, u0, _ = pm.solve_data(op, problem, name, p, inhomogeneous=True)
    w = spla.spsolve(mx.to_scipy((ip, ix, ve)).tocsc(), op.residual(b, u0))
    assert np.all(w[op.fixed] == 0.0)
    u = u0 + w
    rel = np.linalg.norm(op.residual(b, u)) / op.reference_norm(b, u0)
    print(f"{problem} {name} p={p} {layout}: relative residual of the direct solve {rel:.2e}")
    assert rel < 1e-8


def test_csr_apply_statement_on_a_small_matrix():
    """ascending positions, the first product starts the sum, an empty row gives 0.0"""
    from dolfinx_eqlb_amd.lsolver import primal
    ip = np.array([0, 3, 3, 4], dtype=np.int64)
    ix = np.array([0, 1, 2, 1], dtype=np.int32)
    v = np.array([1e16, 1.0, -1e16, -0.0])
    x = np.array([1.0, 1.0, 1.0])
    y, A = primal.csr_apply(ip, ix, v, x, return_abs=True)
    assert y[0] == (1e16 + 1.0) - 1e16 and y[1] == 0.0 and np.signbit(y[2]) and A[0] == 2e16 + 1.0


NEW_SYMBOLS = ("eqlb_primal_matrix_pattern", "eqlb_primal_matrix_export", "eqlb_primal_matrix_values",
               "eqlb_primal_matrix_release", "eqlb_elasticity_matrix_pattern", "eqlb_elasticity_matrix_export",
               "eqlb_elasticity_matrix_values", "eqlb_elasticity_matrix_release", "eqlb_csr_apply")


def test_entries_in_header_library_and_bindings():
    import os
    from dolfinx_eqlb_amd import cpp
    import dolfinx_eqlb_amd._cpp as _cpp
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "eqlb.h")).read()
    L = cpp.lib()
    for s in NEW_SYMBOLS:
        assert s + "(" in text and s in cpp.EXPORTED_SYMBOLS and hasattr(L, s)
    for cls in (cpp.PrimalPoisson, cpp.PrimalElasticity, _cpp.PrimalPoisson, _cpp.PrimalElasticity):
        for m in ("matrix", "matrix_values", "matrix_release"):
            assert hasattr(cls, m)
    assert hasattr(cpp, "csr_apply") and hasattr(_cpp, "csr_apply")


def test_abi_refuses_bad_arguments_before_the_device():
    """the refusals that need no handle and no device: by name, with the code"""
    from dolfinx_eqlb_amd import cpp
    L = cpp.lib()

    def refused(status, who, what):
        assert status == -1
        msg = L.eqlb_last_error().decode()
        assert msg.startswith(who) and what in msg, msg

    n = C.c_int64(0)
    one = np.zeros(4)
    ip = np.array([0, 1], dtype=np.int64)
    ix = np.zeros(1, dtype=np.int32)
    pv, pp, pi = (C.c_void_p(a.ctypes.data) for a in (one, ip, ix))
    host = C.c_int32(cpp.MEM_HOST)
    for pre in ("primal", "elasticity"):
        who = f"eqlb_{pre}_matrix_"
        refused(getattr(L, who + "pattern")(None, C.byref(n), None), who + "pattern", "null")
        refused(getattr(L, who + "export")(None, pp, pi, host, None), who + "export", "null")
        refused(getattr(L, who + "values")(None, C.c_int32(0), pv, C.c_int64(4), host, None), who + "values", "null")
        getattr(L, who + "release")(None)
    ca = L.eqlb_csr_apply
    refused(ca(C.c_int64(1), None, pi, pv, pv, pv, host, None), "eqlb_csr_apply", "null")
    refused(ca(C.c_int64(1), pp, pi, pv, pv, pv, C.c_int32(7), None), "eqlb_csr_apply", "memory space")
    refused(ca(C.c_int64(-1), pp, pi, pv, pv, pv, host, None), "eqlb_csr_apply", "n = -1")
    refused(ca(C.c_int64(2 ** 31), pp, pi, pv, pv, pv, host, None), "eqlb_csr_apply", "n = 2147483648")
    bad = np.array([0, -1], dtype=np.int64)
    refused(ca(C.c_int64(1), C.c_void_p(bad.ctypes.data), pi, pv, pv, pv, host, None), "eqlb_csr_apply", "falls below")
    far = np.array([5], dtype=np.int32)
    refused(ca(C.c_int64(1), pp, C.c_void_p(far.ctypes.data), pv, pv, pv, host, None), "eqlb_csr_apply", "no column")


def test_pattern_planning_stand_alone_under_sanitizers(tmp_path):
    """csrc/eqlb_matrix_plan.h (sizes, sort bits, the guards of the index types) in a program of its own,
    tools/matrix_plan_check.cpp, under AddressSanitizer and UBSan where the compiler has them: the edges of the ranges
    are refused without an overflow on the way, and the figures are the ones worked out here."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "matrix_plan_check")
    base = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", os.path.join(root, "tools", "matrix_plan_check.cpp"),
            "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True,
                         text=True)
    if san.returncode != 0:   # (a compiler without the sanitizer runtimes: the figures are still checked)
        subprocess.run(base, check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.splitlines()
    plans = {tuple(int(v) for v in ln.split("->")[0].split()): [int(v) for v in ln.split("->")[1].split()]
             for ln in lines if "->" in ln and not ln.startswith("bits")}
    i31 = 2 ** 31 - 1
    assert plans[(1, 3, 1, 3)] == [1, 3, 9, 4]                                 # keys 0 ... 8
    assert plans[(1, 15, 1000000, 8004001)] == [1, 8004001, 225000000, (8004001 ** 2 - 1).bit_length()]
    assert plans[(2, 15, 1000000, 8004001)][:3] == [1, 16008002, 225000000]
    assert plans[(1, 3, i31, i31)] == [1, i31, 9 * i31, 62]
    assert plans[(2, 3, 100, i31 // 2)][:2] == [1, i31 - 1]
    assert plans[(2, 3, 100, i31 // 2 + 1)][:2] == [0, i31 + 1]
    assert plans[(1, 3, 100, i31 + 1)][0] == 0 and plans[(1, 3, i31 + 1, 100)][0] == 0
    assert plans[(1, 15, 2 ** 63 - 1, 2 ** 63 - 1)][:3] == [0, 2 ** 63 - 1, 2 ** 63 - 1]
    assert plans[(2, 15, 2 ** 63 - 1, 2 ** 63 - 1)][:3] == [0, 2 ** 63 - 1, 2 ** 63 - 1]
    for bad in ((0, 3, 1, 3), (3, 3, 1, 3), (1, 0, 1, 3), (1, 16, 1, 3), (1, 3, 0, 3), (1, 3, 1, 0), (1, 3, -1, -1)):
        assert plans[bad][0] == 0
    bits = {int(ln.split()[1]): int(ln.split()[3]) for ln in lines if ln.startswith("bits")}
    assert bits == {v: max(v.bit_length(), 1) for v in (0, 1, 2, 3, 255, 256, 2 ** 62 - 1, 2 ** 62, 2 ** 64 - 1)}
    assert [ln for ln in lines if ln.startswith("count")] == ["count 1 1 0 1 0"]
    assert [ln for ln in lines if ln.startswith("kept")] == [f"kept {8 * 8004002 + 8 * 225000000}"]
