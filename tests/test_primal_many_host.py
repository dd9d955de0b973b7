"""Several right-hand sides in one P_p Poisson solve, as far as it can be checked without a device: the numpy statement
(lsolver.primal.PoissonOperator.pcg_many, lsolver.multilevel.Hierarchy.pcg_many) is the loop over the columns of pcg,
the header declares the four *_many entries and the bindings know them."""

import os
import re

import numpy as np
import pytest

import galerkin as gk
import multilevel_cases as mc
import primal_cases as pc
from dolfinx_eqlb_amd.lsolver import primal
from dolfinx_eqlb_amd.lsolver.multilevel import Hierarchy
from dolfinx_eqlb_amd.mesh import create_unit_square

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MANY = ["eqlb_primal_apply_many", "eqlb_primal_solve_many", "eqlb_hierarchy_precondition_many",
        "eqlb_hierarchy_solve_many"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_info(a, b):
    """two info dicts agree key by key; floats by their bits (a NaN column has nb = NaN)"""
    return a.keys() == b.keys() and all(np.array_equal(bits(a[k]), bits(b[k])) for k in a)


def columns(op, rng):
    """B, U [4][ndofs]: nothing to solve, a random system, a system with a NaN in b, a second random system"""
    n = op.ndofs
    g = np.where(op.fixed, rng.standard_normal(n), 0.0)
    B = np.stack([np.zeros(n), rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)])
    B[2, np.nonzero(~op.fixed)[0][5]] = np.nan
    U = np.stack([np.where(op.fixed, 0.0, 1.0), g, g, np.where(op.fixed, g, rng.standard_normal(n))])
    return B, U


@pytest.mark.parametrize("p", [1, 2])
def test_pcg_many_is_the_loop_over_the_columns(p):
    mesh = create_unit_square(4, shuffle_seed=3, perturb=0.15)
    op = primal.PoissonOperator(mesh, p, pc.kappa_of(mesh.ncells))
    op.set_dirichlet(np.concatenate(gk.side_facets(mesh)[:2]))
    B, U = columns(op, np.random.default_rng(p))
    for kw in (dict(rtol=1e-10, maxit=500), dict(rtol=1e-10, maxit=7)):
        X, infos = op.pcg_many(B, U, **kw)
        assert X.shape == B.shape and len(infos) == 4
        for c in range(4):
            x, info = op.pcg(B[c], U[c], **kw)
            assert np.array_equal(bits(X[c]), bits(x)) and same_info(infos[c], info)
    assert infos[0]["converged"] == 1 and infos[0]["iterations"] == 0
    assert infos[2]["breakdown"] == 1 and infos[1]["breakdown"] == 0 and infos[1]["iterations"] == 7
    with pytest.raises(ValueError, match="pcg_many"):
        op.pcg_many(B, U[:3])
    with pytest.raises(ValueError, match="pcg_many"):
        op.pcg_many(B[0], U[0])


def test_hierarchy_pcg_many_is_the_loop_over_the_columns():
    base = create_unit_square(3, shuffle_seed=3, perturb=0.15)
    meshes, links = mc.levels_host(base, [mc.all_cells])
    H = mc.hierarchy(meshes, links, 2, "poisson")[0]
    assert isinstance(H, Hierarchy)
    op = H.ops[-1]
    B, U = columns(op, np.random.default_rng(4))
    X, infos = H.pcg_many(B, U, rtol=1e-10, maxit=200)
    for c in range(4):
        x, info = H.pcg(B[c], U[c], rtol=1e-10, maxit=200)
        assert np.array_equal(bits(X[c]), bits(x)) and same_info(infos[c], info)
    assert infos[1]["converged"] == 1 and infos[2]["breakdown"] == 1
    He = mc.hierarchy(meshes, links, 1, "elasticity")[0]
    n2 = He.ops[-1].fixed.size
    with pytest.raises(ValueError, match="Poisson operator only"):
        He.pcg_many(np.zeros((2, n2)), np.zeros((2, n2)))


def test_header_bindings_and_exports_know_the_many_entries():
    from dolfinx_eqlb_amd import cpp
    text = open(os.path.join(ROOT, "include", "eqlb.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(eqlb_[a-z_0-9]+)\s*\(", text))
    for name in MANY:
        assert name in declared and name in cpp.EXPORTED_SYMBOLS
    assert sorted(declared) == sorted(cpp.EXPORTED_SYMBOLS)
    # every vector argument of the new entries sits behind the column count
    for name in MANY:
        assert re.search(name + r"\(eqlb_[a-z]+_t\* handle, int32_t nrhs, const double\* [a-z], double\* [a-z],", text)
    if os.path.exists(cpp.LIB_PATH):
        for name in MANY:
            assert hasattr(cpp.lib(), name)
    for cls, names in ((cpp.PrimalPoisson, ("apply_many", "apply_many_raw", "solve_many", "solve_many_raw")),
                       (cpp.Multilevel, ("precondition_many", "precondition_many_raw", "solve_many", "solve_many_raw"))):
        for name in names:
            assert callable(getattr(cls, name))
    from dolfinx_eqlb_amd import _cpp
    for cls, names in ((_cpp.PrimalPoisson, ("apply_many", "solve_many")),
                       (_cpp.Multilevel, ("precondition_many", "solve_many"))):
        for name in names:
            assert hasattr(cls, name)
