"""The refinement entries of include/eqlb.h as far as they can be checked without a device: declared in the header,
exported by the library, bound in cpp.py and on the pybind carrier; the refusals that need no mesh."""

import ctypes as C
import os
import re

import numpy as np

INVALID_ARGUMENT = -1
ENTRIES = ("eqlb_mesh_refine_plan", "eqlb_refine_counts", "eqlb_refine_write", "eqlb_refine_create_mesh",
           "eqlb_refine_parent_facets", "eqlb_refine_destroy")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_are_declared_exported_and_bound():
    from dolfinx_eqlb_amd import cpp
    header = open(os.path.join(ROOT, "include", "eqlb.h")).read()
    assert "typedef struct eqlb_refine eqlb_refine_t;" in header
    L = cpp.lib()
    for name in ENTRIES:
        assert re.search(r"^(int|void)\s+" + name + r"\(", header, flags=re.M), name
        assert name in cpp.EXPORTED_SYMBOLS, name
        assert hasattr(L, name), name
    assert L.eqlb_refine_destroy.restype is None
    for name in ("refine", "refine_raw"):
        assert hasattr(cpp.DeviceMesh, name), name
    for name in ("counts", "write_raw", "create_mesh", "parent_facets_raw", "close"):
        assert hasattr(cpp.RefinePlan, name), name
    assert "DeviceMesh.refine" in cpp.mark_doerfler.__doc__
    from dolfinx_eqlb_amd import _cpp
    assert hasattr(_cpp.Mesh, "refine")


def test_statement_is_exported_from_the_mesh_package():
    from dolfinx_eqlb_amd import mesh
    from dolfinx_eqlb_amd.mesh import refine
    assert mesh.refine_longest_edge is refine.refine_longest_edge and mesh.parent_facets is refine.parent_facets


def test_null_arguments_are_refused():
    from dolfinx_eqlb_amd import cpp
    L = cpp.lib()
    marked = np.zeros(4, dtype=np.int32)
    n = np.array([1], dtype=np.int64)
    pm, pn = marked.ctypes.data_as(C.c_void_p), n.ctypes.data_as(C.c_void_p)
    sentinel = 0x5EED5EED
    h = C.c_void_p(sentinel)
    st = L.eqlb_mesh_refine_plan(None, pm, pn, C.c_int64(4), C.c_int32(0), None, C.byref(h))
    assert st == INVALID_ARGUMENT and h.value == sentinel
    assert "eqlb_mesh_refine_plan" in L.eqlb_last_error().decode()
    out = C.c_int32(7)
    assert L.eqlb_refine_counts(None, C.byref(out), None, None, None) == INVALID_ARGUMENT and out.value == 7
    assert L.eqlb_refine_write(None, None, None, pm, None, C.c_int32(0), None) == INVALID_ARGUMENT
    assert L.eqlb_refine_create_mesh(None, None, C.byref(h)) == INVALID_ARGUMENT and h.value == sentinel
    assert L.eqlb_refine_parent_facets(None, None, pm, C.c_int32(0), None) == INVALID_ARGUMENT
    assert "eqlb_refine_parent_facets" in L.eqlb_last_error().decode()
    L.eqlb_refine_destroy(None)   # as free(NULL)
