"""The transfer entries of include/eqlb.h as far as they can be checked without a device: declared in the header,
exported by the library, bound in cpp.py and on the pybind carrier; the refusals that need no mesh."""

import ctypes as C
import os
import re

import numpy as np

INVALID_ARGUMENT = -1
ENTRIES = ("eqlb_mesh_lagrange_dofmap", "eqlb_get_prolong_table", "eqlb_refine_prolong_lagrange",
           "eqlb_refine_prolong_dg")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_are_declared_exported_and_bound():
    import inspect
    from dolfinx_eqlb_amd import cpp
    header = open(os.path.join(ROOT, "include", "eqlb.h")).read()
    L = cpp.lib()
    for name in ENTRIES:
        assert re.search(r"^int\s+" + name + r"\(", header, flags=re.M), name
        assert name in cpp.EXPORTED_SYMBOLS, name
        assert hasattr(L, name), name
    for name in ("lagrange_dofmap", "lagrange_dofmap_raw"):
        assert hasattr(cpp.DeviceMesh, name), name
    for name in ("prolong_lagrange_raw", "prolong_dg_raw"):
        assert hasattr(cpp.RefinePlan, name), name
    for name in ("prolong", "prolong_dg", "close"):
        assert hasattr(cpp.Refinement, name), name
    keep = inspect.signature(cpp.DeviceMesh.refine).parameters["keep_plan"]
    assert keep.default is False
    from dolfinx_eqlb_amd import _cpp
    assert hasattr(_cpp.Mesh, "lagrange_dofmap")
    for name in ("prolong", "prolong_dg"):
        assert hasattr(_cpp.Transfer, name), name
    assert "keep_plan" in _cpp.Mesh.refine.__doc__


def test_statement_is_exported_from_the_mesh_package():
    from dolfinx_eqlb_amd import mesh
    from dolfinx_eqlb_amd.mesh import transfer
    for name in ("lagrange_dofmap", "prolong_table", "prolong_lagrange", "prolong_dg"):
        assert getattr(mesh, name) is getattr(transfer, name), name


def test_null_arguments_are_refused():
    from dolfinx_eqlb_amd import cpp
    L = cpp.lib()
    idx = np.full(12, 3, dtype=np.int32)
    val = np.full(12, 7.0)
    pi, pv = idx.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p)
    n = C.c_int64(-5)
    host = C.c_int32(0)
    one = C.c_int32(1)
    fake = C.c_void_p(0x5EED5EED)   # never dereferenced: the null argument is found first

    assert L.eqlb_mesh_lagrange_dofmap(None, one, pi, C.byref(n), host, None) == INVALID_ARGUMENT
    assert "eqlb_mesh_lagrange_dofmap" in L.eqlb_last_error().decode() and n.value == -5

    nd = C.c_int64(12)
    for plan, refined, cd, u, cd2, u2 in ((None, fake, pi, pv, pi, pv), (fake, None, pi, pv, pi, pv),
                                          (None, None, None, pv, pi, pv), (None, None, pi, None, pi, pv),
                                          (None, None, pi, pv, None, pv), (None, None, pi, pv, pi, None)):
        st = L.eqlb_refine_prolong_lagrange(plan, refined, one, one, one, cd, nd, u, cd2, nd, u2, host, None)
        assert st == INVALID_ARGUMENT
        assert "eqlb_refine_prolong_lagrange" in L.eqlb_last_error().decode()

    for plan, refined, vin, vout in ((None, fake, pv, pv), (fake, None, pv, pv), (None, None, None, pv),
                                     (None, None, pv, None)):
        st = L.eqlb_refine_prolong_dg(plan, refined, one, one, one, vin, vout, host, None)
        assert st == INVALID_ARGUMENT
        assert "eqlb_refine_prolong_dg" in L.eqlb_last_error().decode()
    assert np.all(idx == 3) and np.all(val == 7.0)
