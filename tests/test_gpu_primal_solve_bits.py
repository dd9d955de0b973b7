"""The bits of the P_p solves, pinned to a recording (tests/golden/primal_solve_bits.json).

The numpy statements pin operator, load, diagonal, residual and preconditioner bit for bit, and "many equals single"
(tests/test_gpu_primal_many.py) compares two entries of one implementation.  Neither pins what a SOLVE returns: the order
of every inner product, the scalar steps and the way the host loop batches, replaces and retires.  This module does, for
cases the other modules already build:
  jacobi_p1 ... p4                the 576-cell mesh and the five KINDS columns of tests/test_gpu_primal_many.py at TIGHT,
                                  by PrimalPoisson.solve column by column and by solve_many
  hierarchy_poisson_p1 ... p4     the hierarchy 324 -> 403 -> 1612 cells of tests/test_gpu_multilevel.py (two Dirichlet
                                  sides), the five columns at rtol 1e-12, by Multilevel.solve and by solve_many
  hierarchy_elasticity_p1, p2     the same levels, Dirichlet all around, one random right-hand side, by Multilevel.solve
  elasticity_jacobi_p1 ... p4     the base mesh of tests/test_gpu_primal_elasticity.py, by PrimalElasticity.solve
Per case, entry and column the file holds one line: the sha256 of the bytes of u, then the values of info (keys in
sorted order) as the bits of their float64 (the rule of same_info).  No tolerance.

The file was written by `python tools/record_primal_bits.py` on the device with the library of the commit BEFORE the
single and the many-column paths were folded into one (EQLB_AMD_LIB selects the library; the tool goes through the public
Python API only).  It is regenerated - by the same command, with the library of the tree - only by a change that MEANS to
alter the order of a sum or a rule of the iteration, and that change says so."""

import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "primal_solve_bits.json")


INFO_KEYS = ("breakdown", "converged", "facets_skipped", "iterations", "nb", "replacements", "rnorm", "tol")


def record(u, info):
    """what is kept of one solve, as one line: the digest of u, then the eight values of info in the order of INFO_KEYS"""
    assert tuple(sorted(info)) == INFO_KEYS
    f64 = lambda v: int(np.ascontiguousarray(v, dtype=np.float64).view(np.uint64).ravel()[0])   # noqa: E731
    return " ".join([hashlib.sha256(np.ascontiguousarray(u, dtype=np.float64).tobytes()).hexdigest()]
                    + [f"{f64(info[k]):016x}" for k in INFO_KEYS])


def by_both_entries(solve, solve_many, B, U, **kw):
    X, infos = solve_many(B, U, **kw)
    return dict(solve=[record(*solve(B[c], U[c], **kw)) for c in range(B.shape[0])],
                solve_many=[record(X[c], infos[c]) for c in range(B.shape[0])])


def jacobi(p):
    import test_gpu_primal_many as tm
    h = tm.small(p)["h"]
    B, U = tm.jacobi_columns(p)
    return by_both_entries(h.solve, h.solve_many, B, U, rtol=tm.TIGHT, maxit=20000)


def hierarchy_poisson(p):
    import test_gpu_primal_many as tm
    c = tm.hierarchy("poisson", p, 3, "mixed")
    ml = c["ml"]
    B, U = tm.columns(c["ops"][-1], c["hs"][-1].load, ml.solve, 200 + p, 1e-12)
    return by_both_entries(ml.solve, ml.solve_many, B, U, rtol=1e-12, maxit=5000)


def hierarchy_elasticity(p):
    from test_gpu_multilevel import hierarchy
    c = hierarchy("elasticity", p, 3, "all")
    n = c["ops"][-1].fixed.size
    b = np.random.default_rng(11 * p).standard_normal(n)
    return dict(solve=[record(*c["ml"].solve(b, np.zeros(n), rtol=1e-10, maxit=5000))])


def elasticity_jacobi(p):
    from test_gpu_primal_elasticity import problem
    c = problem("base", p)
    b = c["op"].load(c["d"], c["f"])
    return dict(solve=[record(*c["h"].solve(b, np.zeros(c["n"]), rtol=1e-10, maxit=20000))])


CASES = {f"{fn.__name__}_p{p}": (fn, p)
         for fn, degrees in ((jacobi, (1, 2, 3, 4)), (hierarchy_poisson, (1, 2, 3, 4)), (hierarchy_elasticity, (1, 2)),
                             (elasticity_jacobi, (1, 2, 3, 4)))
         for p in degrees}


def compute(name):
    fn, p = CASES[name]
    return fn(p)


@pytest.mark.parametrize("name", list(CASES))
def test_solve_gives_the_recorded_bits(name):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert tuple(golden["info_keys"]) == INFO_KEYS
    got, want = compute(name), golden["cases"][name]
    assert got.keys() == want.keys()
    for entry in want:
        assert len(got[entry]) == len(want[entry])
        for c, (g, w) in enumerate(zip(got[entry], want[entry])):
            assert g.split()[1:] == w.split()[1:], f"{name}, {entry}, column {c}: info {g.split()[1:]} != {w.split()[1:]}"
            assert g.split()[0] == w.split()[0], f"{name}, {entry}, column {c}: the bits of u differ from the recording"
