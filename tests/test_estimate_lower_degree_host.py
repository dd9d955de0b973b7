"""Estimators and acceptance predicates with DG_d data, 0 <= d <= k-1 (eqlb_se_estimate_dg, eqlb_ev_estimate_dg,
eqlb_oscillation_dg, eqlb_boundary_residual): what can be checked without a device - the ABI, the numpy statement
the device is compared with, and the argument errors that are decided before a device is touched."""

import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from dolfinx_eqlb_amd.eqlb import check_eqlb_conditions as chk
from dolfinx_eqlb_amd.lsolver.projection import embed_dg
from dolfinx_eqlb_amd.mesh import create_unit_square

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("eqlb_se_estimate_dg", "eqlb_ev_estimate_dg", "eqlb_oscillation_dg", "eqlb_boundary_residual")
PAIRS = [(k, d) for k in (1, 2, 3, 4) for d in range(k)]
EQLB_ERR_INVALID_ARGUMENT = -1


def test_new_symbols_declared_and_exported():
    from dolfinx_eqlb_amd import cpp
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eqlb.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(eqlb_[a-z_0-9]+)\s*\(", text))
    if not os.path.exists(cpp.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = cpp.lib()
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in cpp.EXPORTED_SYMBOLS, s
        assert hasattr(lib, s), s


@pytest.mark.parametrize("k,d", PAIRS)
def test_oscillation_statement_at_degree_d(k, d):
    """G in DG_d and its embedding into DG_{k-1} are the same polynomial, so are the two oscillation terms."""
    mesh = create_unit_square(4, shuffle_seed=2, perturb=0.25)
    rng = np.random.default_rng(100 * k + d)
    nd = (d + 1) * (d + 2) // 2
    x = rng.standard_normal(mesh.ncells * k * (k + 2))
    G = rng.standard_normal(mesh.ncells * nd * 2)
    korn = 1.0 + rng.random(mesh.ncells)

    def f(xx, yy):
        return np.sin(3.0 * xx) * np.exp(yy) + xx * yy
    low = chk.oscillation_term(mesh, k, x, G, f, 8, korn, degree_dg=d)
    emb = chk.oscillation_term(mesh, k, x, embed_dg(G, mesh.ncells, d, k - 1, bs=2), f, 8, korn)
    assert low.shape == (mesh.ncells,) and np.all(low > 0.0)
    assert np.allclose(low, emb, rtol=1e-12, atol=0.0)
    if d == 0 and k > 1:  # a constant G has no divergence
        assert np.allclose(low, chk.oscillation_term(mesh, k, x, None, f, 8, korn), rtol=1e-12, atol=0.0)


def _fake_device_mesh(mesh):
    """What the argument checks of cpp.estimate & co. look at; the handle is never reached."""
    return types.SimpleNamespace(mesh=mesh, _h=None)


def test_argument_errors_before_the_device():
    from dolfinx_eqlb_amd import cpp
    mesh = create_unit_square(2)
    dm = _fake_device_mesh(mesh)
    k, d = 3, 1
    nrt, nd, ndk = k * (k + 2), 3, 6
    x = np.zeros((1, mesh.ncells * nrt))
    G, f = np.zeros((1, mesh.ncells * nd * 2)), np.zeros((1, mesh.ncells * nd))
    qp, qw = np.array([[1 / 3, 1 / 3]]), np.array([0.5])
    fv = np.zeros((1, mesh.ncells, 1))
    # a degree outside 0 ... k-1: the reference's message (se/reconstruction.hpp:363-373)
    for bad in (-1, k, 7):
        with pytest.raises(RuntimeError, match="Wrong polynomial degree"):
            cpp.estimate(dm, k, x, G, f, degree_dg=bad)
        with pytest.raises(RuntimeError, match="Wrong polynomial degree"):
            cpp.oscillation(dm, k, x, G, qp, qw, fv, degree_dg=bad)
        with pytest.raises(RuntimeError, match="Wrong polynomial degree"):
            cpp.boundary_residual(dm, k, x, G, [0], degree_dg=bad)
    with pytest.raises(RuntimeError, match="outside 1 ... 4"):
        cpp.estimate(dm, 5, x, G, f, degree_dg=1)
    # sizes: DG_d data where degree_dg says otherwise, and today's error without degree_dg
    for deg in (None, 0, 2):
        with pytest.raises(RuntimeError, match="sizes"):
            cpp.estimate(dm, k, x, G, f, degree_dg=deg)
        with pytest.raises(RuntimeError, match="sizes"):
            cpp.oscillation(dm, k, x, G, qp, qw, fv, degree_dg=deg)
        with pytest.raises(RuntimeError, match="sizes"):
            cpp.boundary_residual(dm, k, x, G, [0], degree_dg=deg)
    with pytest.raises(RuntimeError, match="sizes"):
        cpp.estimate(dm, k, x, G, np.zeros((1, mesh.ncells * ndk)), degree_dg=d)
    with pytest.raises(RuntimeError, match="sizes"):
        cpp.boundary_residual(dm, k, x, G, [0], boundary_values=np.zeros(3), degree_dg=d)
    for bad in ([-1], [mesh.nfacets], [0, 10 ** 6]):
        with pytest.raises(RuntimeError, match="outside the mesh"):
            cpp.boundary_residual(dm, k, x, G, bad, degree_dg=d)


def test_c_abi_rejects_a_null_mesh():
    """The library itself: no handle, no launch - EQLB_ERR_INVALID_ARGUMENT with a message."""
    from dolfinx_eqlb_amd import cpp
    lib = cpp.lib()
    i32, null = C.c_int32, None
    calls = {
        "eqlb_se_estimate_dg": (null, i32(2), i32(0), i32(1), null, null, null, null, null, null, i32(0), null),
        "eqlb_ev_estimate_dg": (null, i32(2), i32(0), i32(1), null, null, null, null, null, null, i32(0), null),
        "eqlb_oscillation_dg": (null, i32(2), i32(0), i32(1), null, null, i32(1), null, null, null, null, null,
                                i32(0), null),
        "eqlb_boundary_residual": (null, i32(2), i32(0), i32(1), null, null, i32(0), null, null, null, i32(0), null),
    }
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == EQLB_ERR_INVALID_ARGUMENT, name
        assert b"invalid argument" in lib.eqlb_last_error(), name
