"""eqlb_mesh_create_from_cells and the entries around it, as far as they can be checked without a device: the
refusals that come before the device check, the loud failure without a device, the names on the pybind carrier."""

import ctypes as C

import numpy as np
import pytest

INVALID_ARGUMENT = -1
INT32_MAX = 2 ** 31 - 1


def _call(nnodes, ncells, x, cells, memspace, handle):
    from dolfinx_eqlb_amd import cpp
    L = cpp.lib()
    st = L.eqlb_mesh_create_from_cells(C.c_int32(nnodes), C.c_int32(ncells),
                                       None if x is None else x.ctypes.data_as(C.c_void_p),
                                       None if cells is None else cells.ctypes.data_as(C.c_void_p),
                                       C.c_int32(memspace), None, handle)
    return int(st), L.eqlb_last_error().decode()


def test_refusals_before_the_device_check():
    x = np.zeros((3, 3))
    x[1, 0] = x[2, 1] = 1.0
    cells = np.array([[0, 1, 2]], dtype=np.int32)
    h = C.c_void_p()
    cases = {
        "null x": (3, 1, None, cells, 0, C.byref(h)),
        "null cells": (3, 1, x, None, 0, C.byref(h)),
        "null handle": (3, 1, x, cells, 0, None),
        "no nodes": (0, 1, x, cells, 0, C.byref(h)),
        "no cells": (3, 0, x, cells, 0, C.byref(h)),
        "negative count": (3, -1, x, cells, 0, C.byref(h)),
        "memspace 2": (3, 1, x, cells, 2, C.byref(h)),
        "memspace -1": (3, 1, x, cells, -1, C.byref(h)),
        # nothing is read before this check: the arrays need not have that size
        "3 ncells > INT32_MAX": (3, INT32_MAX // 3 + 1, x, cells, 0, C.byref(h)),
        "ncells = INT32_MAX": (3, INT32_MAX, x, cells, 1, C.byref(h)),
    }
    for name, args in cases.items():
        st, msg = _call(*args)
        assert st == INVALID_ARGUMENT, (name, st, msg)
        assert msg and "eqlb_mesh_create_from_cells" in msg, (name, msg)
        assert not h.value, name


def test_small_entries_refuse_a_null_mesh():
    from dolfinx_eqlb_amd import cpp
    L = cpp.lib()
    n = C.c_int32(7)
    out = np.zeros(4, dtype=np.int32)
    p = out.ctypes.data_as(C.c_void_p)
    for name, st in (
            ("eqlb_mesh_counts", L.eqlb_mesh_counts(None, C.byref(n), None, None)),
            ("eqlb_mesh_export", L.eqlb_mesh_export(None, p, None, None, None, None, None, None, None, None,
                                                    C.c_int32(0), None)),
            ("eqlb_mesh_boundary_facets", L.eqlb_mesh_boundary_facets(None, p, C.c_int32(4), C.byref(n), C.c_int32(0),
                                                                      None)),
            ("eqlb_mesh_find_facets", L.eqlb_mesh_find_facets(None, C.c_int32(2), p, p, C.c_int32(0), None))):
        assert st == INVALID_ARGUMENT, name
    assert "eqlb_mesh_find_facets" in L.eqlb_last_error().decode()


def test_from_cells_without_a_device_fails_loudly():
    """Valid arguments and no device: an error, never a host fallback (as test_abi.test_no_device_fails_loudly)."""
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.mesh import create_unit_square
    if cpp.device_count() > 0:
        pytest.skip("a device is visible")
    m = create_unit_square(2)
    with pytest.raises(RuntimeError, match="eqlb_mesh_create_from_cells"):
        cpp.DeviceMesh.from_cells(m.x[:, :2], m.cell_nodes)


def test_pybind_carrier_has_the_new_names():
    from dolfinx_eqlb_amd import _cpp
    for name in ("from_cells", "boundary_facets", "find_facets"):
        assert hasattr(_cpp.Mesh, name), name
    if _cpp.device_count() == 0:
        m = np.array([[0, 1, 2]], dtype=np.int32)
        with pytest.raises(RuntimeError):
            _cpp.Mesh.from_cells(np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]), m)
    with pytest.raises(RuntimeError, match="from_cells"):
        _cpp.Mesh.from_cells(np.zeros((3, 4)), np.array([[0, 1, 2]], dtype=np.int32))
