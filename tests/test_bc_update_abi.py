"""C ABI of the in-place update of flux boundary values (include/eqlb.h: eqlb_facet_points, eqlb_flux_bc_dofs,
eqlb_se_update_flux_bc / eqlb_ev_update_flux_bc, eqlb_*_get_boundary_values): the symbols are exported, and the
argument checks answer before any device call - there is no GPU on the CPU test box, so every call here has to
return from the checks alone."""

import ctypes as C

import numpy as np
import pytest

NEW_SYMBOLS = ["eqlb_facet_points", "eqlb_flux_bc_dofs", "eqlb_se_update_flux_bc", "eqlb_ev_update_flux_bc",
               "eqlb_se_get_boundary_values", "eqlb_ev_get_boundary_values"]
INVALID = -1  # EQLB_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def L():
    from dolfinx_eqlb_amd import cpp
    return cpp.lib()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


S = np.array([0.25, 0.75])
W = np.array([0.5, 0.5])
S65 = np.linspace(0.0, 1.0, 65)
ONE = np.zeros(8, dtype=np.int32)
VAL = np.zeros(1024)


def test_symbols_are_exported(L):
    from dolfinx_eqlb_amd import cpp
    for s in NEW_SYMBOLS:
        assert s in cpp.EXPORTED_SYMBOLS and hasattr(L, s), s
    for name in ("facet_points", "facet_points_raw", "flux_bc_dofs", "flux_bc_dofs_raw"):
        assert callable(getattr(cpp, name))
    for cls in (cpp.SemiExplicitEquilibrator, cpp.ConstrainedMinEquilibrator):
        for name in ("update_flux_bc", "update_flux_bc_raw", "get_boundary_values", "get_boundary_values_raw"):
            assert callable(getattr(cls, name)), (cls, name)


def _refused(L, status, *words):
    assert status == INVALID
    msg = L.eqlb_last_error().decode()
    for w in words:
        assert w in msg, msg


def test_facet_points_argument_checks(L):
    fp = L.eqlb_facet_points
    _refused(L, fp(None, 1, _p(ONE), 2, _p(S), _p(VAL), 0, None), "eqlb_facet_points", "null mesh")
    _refused(L, fp(None, -1, _p(ONE), 2, _p(S), _p(VAL), 0, None), "nlist = -1")
    _refused(L, fp(None, 1, _p(ONE), 65, _p(S65), _p(VAL), 0, None), "nq = 65")
    _refused(L, fp(None, 1, _p(ONE), 0, _p(S), _p(VAL), 0, None), "nq = 0")
    _refused(L, fp(None, 1, _p(ONE), 2, _p(np.array([0.5, 1.5])), _p(VAL), 0, None), "s[1]")
    _refused(L, fp(None, 1, _p(ONE), 2, _p(S), _p(VAL), 7, None), "memory space")


def test_flux_bc_dofs_argument_checks(L):
    fd = L.eqlb_flux_bc_dofs
    args = (_p(ONE), 2, _p(S), _p(W), _p(VAL), 0, _p(VAL), 0, None)
    _refused(L, fd(None, 2, 1, *args), "eqlb_flux_bc_dofs", "null mesh")
    for k in (0, 5, -1):
        _refused(L, fd(None, k, 1, *args), "k = %d" % k)
    _refused(L, fd(None, 2, -3, *args), "nlist = -3")
    _refused(L, fd(None, 2, 1, _p(ONE), 65, _p(S65), _p(S65), _p(VAL), 0, _p(VAL), 0, None), "nq = 65")
    _refused(L, fd(None, 2, 1, _p(ONE), 2, _p(S), _p(W), _p(VAL), 2, _p(VAL), 0, None), "vector")


@pytest.mark.parametrize("name", ["eqlb_se_update_flux_bc", "eqlb_ev_update_flux_bc"])
def test_update_argument_checks(L, name):
    up = getattr(L, name)
    _refused(L, up(None, 0, 1, _p(ONE), 2, _p(S), _p(W), _p(VAL), 0, None, 0, None), name, "null handle")
    _refused(L, up(None, 0, 1, _p(ONE), 0, None, None, _p(VAL), 0, None, 1, None), name, "null handle")
    _refused(L, up(None, 0, -1, _p(ONE), 2, _p(S), _p(W), _p(VAL), 0, None, 0, None), "nlist = -1")
    _refused(L, up(None, 0, 1, _p(ONE), 65, _p(S65), _p(S65), _p(VAL), 0, None, 0, None), "nq = 65")
    _refused(L, up(None, 0, 1, _p(ONE), -1, _p(S), _p(W), _p(VAL), 0, None, 0, None), "nq = -1")


@pytest.mark.parametrize("name", ["eqlb_se_get_boundary_values", "eqlb_ev_get_boundary_values"])
def test_get_boundary_values_argument_checks(L, name):
    _refused(L, getattr(L, name)(None, _p(VAL), 0, None), name, "null")


def test_binding_checks_sizes_before_the_library():
    """The numpy front ends refuse arrays of the wrong size themselves (no handle, no device needed)."""
    from dolfinx_eqlb_amd import cpp

    class Fake:
        k, nrhs, _h = 2, 1, None

    with pytest.raises(RuntimeError, match="sizes"):
        cpp._update_flux_bc(None, Fake(), 0, [1, 2, 3], np.zeros(5), None, None, False)
    with pytest.raises(RuntimeError, match="weights"):
        cpp._update_flux_bc(None, Fake(), 0, [1, 2, 3], np.zeros(6), S, None, False)
