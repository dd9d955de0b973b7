"""ctypes binding of libeqlb_amd.so (include/eqlb.h) - the stand-in for the reference's
pybind11 module `dolfinx_eqlb.cpp` (python/dolfinx_eqlb/wrappers.cpp:259-272).

The product path has no CPU fallback: if the HIP library is missing or no device is visible,
the calls raise.  Errors of the C ABI are raised as RuntimeError, like the reference's
std::runtime_error -> RuntimeError translation.
"""

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EQLB_AMD_LIB", os.path.join(_HERE, "libeqlb_amd.so"))

MEM_HOST, MEM_DEVICE = 0, 1
SOLVER_LDS_CHOLESKY, SOLVER_SHUFFLE = 0, 1
SCATTER_SLOTS, SCATTER_ATOMIC, SCATTER_TILED = 0, 1, 2

# every symbol include/eqlb.h declares (tests check that the library exports all of them)
EXPORTED_SYMBOLS = [
    "eqlb_last_error", "eqlb_device_count", "eqlb_mesh_create", "eqlb_mesh_destroy",
    "eqlb_mesh_max_patch_cells", "eqlb_se_create", "eqlb_se_destroy", "eqlb_se_set_option",
    "eqlb_se_set_boundary", "eqlb_se_equilibrate", "eqlb_se_num_patches",
    "eqlb_se_export_patches", "eqlb_get_reference_table", "eqlb_se_last_kernel_ms",
    "eqlb_project_dg", "eqlb_se_equilibrate_with_kornconst",
    "eqlb_ev_create", "eqlb_ev_destroy", "eqlb_ev_set_option", "eqlb_ev_set_dofmap",
    "eqlb_ev_num_dofs", "eqlb_ev_set_boundary", "eqlb_ev_equilibrate", "eqlb_ev_num_patches",
    "eqlb_ev_last_kernel_ms", "eqlb_se_tiling_info", "eqlb_se_estimate",
    "eqlb_halo_pack", "eqlb_halo_unpack_add", "eqlb_ev_estimate",
    "eqlb_se_check_status", "eqlb_ev_check_status",
    "eqlb_se_set_priority_cells", "eqlb_se_num_priority_tiles", "eqlb_se_equilibrate_tiles",
    "eqlb_se_equilibrate_lists", "eqlb_ev_equilibrate_lists", "eqlb_se_kornconst",
    "eqlb_ev_set_basis_transform", "eqlb_se_estimate_stress", "eqlb_oscillation",
    "eqlb_halo_exchange", "eqlb_halo_reduce", "eqlb_rccl_get_unique_id", "eqlb_rccl_comm_create",
    "eqlb_rccl_comm_destroy", "eqlb_halo_create", "eqlb_halo_destroy", "eqlb_halo_bytes", "eqlb_halo_reduce_plan",
    "eqlb_se_tiling_blocks", "eqlb_ev_tiling_blocks", "eqlb_ev_create_dg",
    "eqlb_se_estimate_dg", "eqlb_ev_estimate_dg", "eqlb_oscillation_dg", "eqlb_boundary_residual",
    "eqlb_se_large_patch_info", "eqlb_ev_large_patch_info",
    "eqlb_indicator_total", "eqlb_mark_doerfler",
    "eqlb_primal_flux_dg", "eqlb_primal_stress_dg", "eqlb_get_primal_table",
    "eqlb_facet_points", "eqlb_flux_bc_dofs", "eqlb_se_update_flux_bc", "eqlb_ev_update_flux_bc",
    "eqlb_se_get_boundary_values", "eqlb_ev_get_boundary_values",
    "eqlb_mesh_create_from_cells", "eqlb_mesh_counts", "eqlb_mesh_export", "eqlb_mesh_boundary_facets",
    "eqlb_mesh_find_facets",
    "eqlb_mesh_refine_plan", "eqlb_refine_counts", "eqlb_refine_write", "eqlb_refine_create_mesh",
    "eqlb_refine_parent_facets", "eqlb_refine_destroy",
    "eqlb_mesh_lagrange_dofmap", "eqlb_get_prolong_table", "eqlb_refine_prolong_lagrange", "eqlb_refine_prolong_dg",
    "eqlb_refine_facet_types", "eqlb_refine_child_facets", "eqlb_get_flux_bc_prolong_table",
    "eqlb_refine_prolong_flux_bc", "eqlb_se_carry_boundary", "eqlb_ev_carry_boundary",
    "eqlb_get_stiffness_table", "eqlb_get_load_table", "eqlb_primal_create", "eqlb_primal_destroy",
    "eqlb_primal_ndofs", "eqlb_primal_set_dirichlet", "eqlb_primal_load", "eqlb_primal_apply",
    "eqlb_primal_diagonal", "eqlb_primal_residual", "eqlb_primal_solve",
    "eqlb_get_cross_table", "eqlb_elasticity_create", "eqlb_elasticity_destroy", "eqlb_elasticity_ndofs",
    "eqlb_elasticity_set_dirichlet", "eqlb_elasticity_load", "eqlb_elasticity_apply", "eqlb_elasticity_diagonal",
    "eqlb_elasticity_residual", "eqlb_elasticity_solve",
    "eqlb_hierarchy_create", "eqlb_hierarchy_destroy", "eqlb_hierarchy_restrict", "eqlb_hierarchy_precondition",
    "eqlb_hierarchy_solve",
    "eqlb_primal_apply_many", "eqlb_primal_solve_many", "eqlb_hierarchy_precondition_many",
    "eqlb_hierarchy_solve_many",
    "eqlb_hierarchy_set_local", "eqlb_hierarchy_active", "eqlb_hierarchy_active_count",
    "eqlb_hierarchy_set_coarse", "eqlb_hierarchy_coarse_rows", "eqlb_hierarchy_coarse_factor",
    "eqlb_get_mass_table", "eqlb_primal_set_reaction", "eqlb_elasticity_set_reaction",
    "eqlb_primal_value_dg", "eqlb_get_value_table",
    "eqlb_elasticity_set_shear", "eqlb_primal_stress_dg_mu", "eqlb_se_estimate_stress_mu",
    "eqlb_primal_set_diffusion", "eqlb_primal_flux_dg_tensor", "eqlb_se_estimate_weighted", "eqlb_ev_estimate_weighted",
    "eqlb_primal_matrix_pattern", "eqlb_primal_matrix_export", "eqlb_primal_matrix_values", "eqlb_primal_matrix_release",
    "eqlb_elasticity_matrix_pattern", "eqlb_elasticity_matrix_export", "eqlb_elasticity_matrix_values",
    "eqlb_elasticity_matrix_release", "eqlb_csr_apply",
    "eqlb_get_facet_mass_table", "eqlb_primal_set_robin", "eqlb_primal_robin_weights", "eqlb_primal_robin_flux",
    "eqlb_elasticity_set_springs", "eqlb_elasticity_spring_weights", "eqlb_elasticity_spring_flux",
]

# eqlb_se_tiling_blocks: per bin (P = 4, 8, 16, 32, 64) the wave-blocks of each body instance and the padding copies,
# in the order of EQLB_TB_FULL ... EQLB_TB_PADDING; then the tiles with the zero flag (EQLB_TB_ZERO_TILES)
TILING_BLOCK_KINDS = ("full", "interior", "nfix1", "nfix2", "nfix3", "generic", "padding")
_TB_COUNT = 5 * len(TILING_BLOCK_KINDS) + 1


def _tiling_blocks(fn, h):
    """dict kind -> [count per bin 0 ... 4] (TILING_BLOCK_KINDS), and "zero_tiles" -> int."""
    out = (C.c_int64 * _TB_COUNT)()
    _check(fn(h, out, C.c_int32(_TB_COUNT)))
    v = [int(x) for x in out]
    nk = len(TILING_BLOCK_KINDS)
    d = {kind: [v[nk * b + i] for b in range(5)] for i, kind in enumerate(TILING_BLOCK_KINDS)}
    d["zero_tiles"] = v[5 * nk]
    return d

def _large_patch_info(fn, h):
    """(number of patches on the large-patch kernel, cells of the largest one)."""
    n, mx = C.c_int64(0), C.c_int32(0)
    _check(fn(h, C.byref(n), C.byref(mx)))
    return int(n.value), int(mx.value)


def _rule(s, w=None):
    """Facet rule as host arrays: parameters s in [0, 1] and (optionally) weights w on [0, 1]."""
    ss = np.ascontiguousarray(s, dtype=np.float64).ravel()
    ww = None if w is None else np.ascontiguousarray(w, dtype=np.float64).ravel()
    if ww is not None and ww.size != ss.size:
        raise RuntimeError("Equilibration: Input sizes does not match")
    return ss, ww


def _update_flux_bc(fn, eq, rhs, facets, values, s, w, vector):
    """Host arrays -> eqlb_*_update_flux_bc: values [nlist, k] facet DOFs (s is None), point values [nlist, nq]
    of the normal flux, or [nlist, nq, 2] of a vector field (vector=True)."""
    fl = np.ascontiguousarray(facets, dtype=np.int32).ravel()
    v = np.ascontiguousarray(values, dtype=np.float64)
    if s is None:
        nq, ss, ww = 0, None, None
        need = fl.size * eq.k
    else:
        ss, ww = _rule(s, w)
        if ww is None:
            raise RuntimeError("Equilibration: point values need the weights of the facet rule")
        nq = ss.size
        need = fl.size * nq * (2 if vector else 1)
    if v.size != need:
        raise RuntimeError("Equilibration: Input sizes does not match")
    _check(fn(eq._h, C.c_int32(rhs), C.c_int32(fl.size), _hp(fl), C.c_int32(nq),
              _hp(ss) if ss is not None else None, _hp(ww) if ww is not None else None, _hp(v),
              C.c_int32(1 if vector else 0), None, C.c_int32(MEM_HOST), None))


def _update_flux_bc_raw(fn, eq, rhs, nlist, facets, values, s, w, vector, nrejected, memspace, stream):
    if s is None:
        nq, ss, ww = 0, None, None
    else:
        ss, ww = _rule(s, w)
        nq = ss.size
    _check(fn(eq._h, C.c_int32(rhs), C.c_int32(nlist), _vp(facets), C.c_int32(nq),
              _hp(ss) if ss is not None else None, _hp(ww) if ww is not None else None, _vp(values),
              C.c_int32(1 if vector else 0), _vp(nrejected), C.c_int32(memspace), C.c_void_p(stream)))


def _carry_boundary(fn, eq, old, refinement, node_mask, stream):
    plan = refinement._kept_plan("carry_boundary")
    nm = None
    if node_mask is not None:
        nm = np.ascontiguousarray(node_mask, dtype=np.uint8)
        if nm.size != refinement.counts["nnodes2"]:
            raise RuntimeError("carry_boundary: Input sizes does not match")
    _check(fn(old._h, plan._h, eq._h, _hp(nm) if nm is not None else None, C.c_void_p(stream)))


def _get_boundary_values(fn, eq):
    out = np.zeros((eq.nrhs, eq.dmesh.mesh.ncells * eq.nrt))
    _check(fn(eq._h, _hp(out), C.c_int32(MEM_HOST), None))
    return out


_lib = None


def _bind_torch_hip_runtime():
    """torch bundles its own HIP runtime (torch/lib/libamdhip64.so, same soname as /opt/rocm's).  Two
    runtimes in one process do not share devices: the one initialised second sees none.  Callers that
    hand torch tensors to this library (bench.py, distributed.HaloExchange) therefore need ONE runtime,
    torch's.  If torch is installed but not imported yet, its runtime is mapped first (without importing
    torch), so that libeqlb_amd.so binds to it and a later `import torch` finds it already loaded."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass  # a torch build without a usable bundled runtime: the system runtime is used


def lib():
    """Load libeqlb_amd.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()')")
        _bind_torch_hip_runtime()
        L = C.CDLL(LIB_PATH)
        L.eqlb_last_error.restype = C.c_char_p
        L.eqlb_device_count.restype = C.c_int
        L.eqlb_se_num_patches.restype = C.c_int64
        L.eqlb_se_last_kernel_ms.restype = C.c_double
        L.eqlb_mesh_max_patch_cells.restype = C.c_int32
        L.eqlb_ev_num_dofs.restype = C.c_int64
        L.eqlb_ev_num_patches.restype = C.c_int64
        L.eqlb_ev_last_kernel_ms.restype = C.c_double
        for name in ("eqlb_mesh_destroy", "eqlb_se_destroy", "eqlb_ev_destroy", "eqlb_halo_destroy",
                     "eqlb_rccl_comm_destroy"):
            getattr(L, name).restype = None
        for name in ("eqlb_refine_destroy", "eqlb_primal_destroy", "eqlb_elasticity_destroy", "eqlb_hierarchy_destroy",
                     "eqlb_primal_matrix_release", "eqlb_elasticity_matrix_release"):
            if hasattr(L, name):   # (a library of an earlier revision, EQLB_AMD_LIB: A/B runs of bench.py)
                getattr(L, name).restype = None
        _lib = L
    return _lib


def _check(status):
    if status != 0:
        raise RuntimeError(lib().eqlb_last_error().decode() or f"eqlb error {status}")


def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


def device_count() -> int:
    return int(lib().eqlb_device_count())


class DeviceMesh:
    """Device-resident copy of a flat mesh (eqlb_mesh_create)."""

    def __init__(self, mesh):
        self.mesh = mesh
        self._h = C.c_void_p()
        arrs = [np.ascontiguousarray(mesh.x, dtype=np.float64),
                np.ascontiguousarray(mesh.cell_nodes, dtype=np.int32),
                np.ascontiguousarray(mesh.cell_facets, dtype=np.int32),
                np.ascontiguousarray(mesh.facet_nodes, dtype=np.int32),
                np.ascontiguousarray(mesh.facet_cells_offsets, dtype=np.int32),
                np.ascontiguousarray(mesh.facet_cells, dtype=np.int32),
                np.ascontiguousarray(mesh.node_cells_offsets, dtype=np.int32),
                np.ascontiguousarray(mesh.node_cells, dtype=np.int32),
                np.ascontiguousarray(mesh.node_facets_offsets, dtype=np.int32),
                np.ascontiguousarray(mesh.node_facets, dtype=np.int32),
                np.ascontiguousarray(mesh.facet_perm, dtype=np.uint8)]
        _check(lib().eqlb_mesh_create(C.c_int32(mesh.nnodes), C.c_int32(mesh.ncells),
                                      C.c_int32(mesh.nfacets), *[_hp(a) for a in arrs],
                                      C.byref(self._h)))

    @classmethod
    def from_cells(cls, x, cell_nodes, device=False, stream=0):
        """eqlb_mesh_create_from_cells: the connectivity is built on the device from the coordinates and the cells
        alone, in the numbering of mesh.create_mesh; `.mesh` is filled from eqlb_mesh_export.
        device=False: host arrays, x [n, 2] or [n, 3].  device=True: x [n, 3] float64 and cell_nodes [m, 3] int32 are
        contiguous torch tensors on the device (their data_ptr() is handed over), read on `stream`."""
        from .mesh import Mesh
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        self.mesh = None
        if device:
            if tuple(x.shape[1:]) != (3,) or tuple(cell_nodes.shape[1:]) != (3,) \
                    or not x.is_contiguous() or not cell_nodes.is_contiguous() \
                    or x.element_size() != 8 or cell_nodes.element_size() != 4:
                raise RuntimeError("DeviceMesh.from_cells: contiguous x [n, 3] float64 and cell_nodes [m, 3] int32 expected")
            nnodes, ncells = int(x.shape[0]), int(cell_nodes.shape[0])
            px, pc = C.c_void_p(x.data_ptr()), C.c_void_p(cell_nodes.data_ptr())
        else:
            x2 = np.asarray(x, dtype=np.float64)
            if x2.ndim != 2 or x2.shape[1] not in (2, 3):
                raise RuntimeError("DeviceMesh.from_cells: x [n, 2] or [n, 3] expected")
            hx = np.zeros((x2.shape[0], 3))
            hx[:, :x2.shape[1]] = x2
            hc = np.ascontiguousarray(cell_nodes, dtype=np.int32)
            if hc.ndim != 2 or hc.shape[1] != 3:
                raise RuntimeError("DeviceMesh.from_cells: cell_nodes [m, 3] expected")
            nnodes, ncells = hx.shape[0], hc.shape[0]
            px, pc = _hp(hx), _hp(hc)
        _check(lib().eqlb_mesh_create_from_cells(C.c_int32(nnodes), C.c_int32(ncells), px, pc,
                                                 C.c_int32(MEM_DEVICE if device else MEM_HOST), C.c_void_p(stream),
                                                 C.byref(self._h)))
        if device:
            hx = x.cpu().numpy().astype(np.float64, copy=False)
            hc = cell_nodes.cpu().numpy().astype(np.int32, copy=False)
        t = self.export()
        self.mesh = Mesh(hx, hc, t["cell_facets"], t["facet_nodes"], t["facet_cells_offsets"], t["facet_cells"],
                         t["node_cells_offsets"], t["node_cells"], t["node_facets_offsets"], t["node_facets"],
                         t["facet_perm"])
        return self

    def counts(self):
        """(nnodes, ncells, nfacets) of the handle (eqlb_mesh_counts)."""
        v = [C.c_int32(0) for _ in range(3)]
        _check(lib().eqlb_mesh_counts(self._h, *[C.byref(a) for a in v]))
        return tuple(int(a.value) for a in v)

    def export(self):
        """The tables of the handle as host arrays (eqlb_mesh_export), by the field names of mesh.Mesh."""
        nn, nc, nf = self.counts()
        off = {"facet_cells_offsets": np.zeros(nf + 1, dtype=np.int32),
               "node_cells_offsets": np.zeros(nn + 1, dtype=np.int32),
               "node_facets_offsets": np.zeros(nn + 1, dtype=np.int32)}
        _check(lib().eqlb_mesh_export(self._h, None, None, _hp(off["facet_cells_offsets"]), None,
                                      _hp(off["node_cells_offsets"]), None, _hp(off["node_facets_offsets"]), None,
                                      None, C.c_int32(MEM_HOST), None))
        t = {"cell_facets": np.zeros((nc, 3), dtype=np.int32), "facet_nodes": np.zeros((nf, 2), dtype=np.int32),
             "facet_cells": np.zeros(int(off["facet_cells_offsets"][-1]), dtype=np.int32),
             "node_cells": np.zeros(int(off["node_cells_offsets"][-1]), dtype=np.int32),
             "node_facets": np.zeros(int(off["node_facets_offsets"][-1]), dtype=np.int32),
             "facet_perm": np.zeros((nc, 3), dtype=np.uint8)}
        _check(lib().eqlb_mesh_export(self._h, _hp(t["cell_facets"]), _hp(t["facet_nodes"]), None,
                                      _hp(t["facet_cells"]), None, _hp(t["node_cells"]), None, _hp(t["node_facets"]),
                                      _hp(t["facet_perm"]), C.c_int32(MEM_HOST), None))
        t.update(off)
        return t

    def export_raw(self, cell_facets=None, facet_nodes=None, facet_cells_offsets=None, facet_cells=None,
                   node_cells_offsets=None, node_cells=None, node_facets_offsets=None, node_facets=None,
                   facet_perm=None, memspace=MEM_DEVICE, stream=0):
        """eqlb_mesh_export on raw pointers (ints, None for a table that is not wanted) in `memspace`."""
        _check(lib().eqlb_mesh_export(self._h, _vp(cell_facets), _vp(facet_nodes), _vp(facet_cells_offsets),
                                      _vp(facet_cells), _vp(node_cells_offsets), _vp(node_cells),
                                      _vp(node_facets_offsets), _vp(node_facets), _vp(facet_perm),
                                      C.c_int32(memspace), C.c_void_p(stream)))

    def boundary_facets(self):
        """Ids of the facets with one cell, ascending (eqlb_mesh_boundary_facets)."""
        n = C.c_int32(0)
        out = np.zeros(self.counts()[2], dtype=np.int32)
        _check(lib().eqlb_mesh_boundary_facets(self._h, _hp(out), C.c_int32(out.size), C.byref(n),
                                               C.c_int32(MEM_HOST), None))
        return out[:n.value].copy()

    def boundary_facets_raw(self, facets, capacity, memspace=MEM_DEVICE, stream=0):
        """eqlb_mesh_boundary_facets on a raw pointer; returns (status, count) - the count is reported even when the
        capacity is refused."""
        n = C.c_int32(0)
        st = lib().eqlb_mesh_boundary_facets(self._h, _vp(facets), C.c_int32(capacity), C.byref(n),
                                             C.c_int32(memspace), C.c_void_p(stream))
        return int(st), int(n.value)

    def find_facets(self, pairs):
        """Facet id of every node pair [npairs, 2] in either order, -1 where the pair is no edge of the mesh
        (eqlb_mesh_find_facets): translates facets tagged by their vertices into the ids of facet_type."""
        p = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        out = np.zeros(p.shape[0], dtype=np.int32)
        _check(lib().eqlb_mesh_find_facets(self._h, C.c_int32(p.shape[0]), _hp(p), _hp(out), C.c_int32(MEM_HOST),
                                           None))
        return out

    def find_facets_raw(self, npairs, pairs, facets, memspace=MEM_DEVICE, stream=0):
        _check(lib().eqlb_mesh_find_facets(self._h, C.c_int32(npairs), _vp(pairs), _vp(facets), C.c_int32(memspace),
                                           C.c_void_p(stream)))

    def lagrange_dofmap_raw(self, p, cell_dofs, memspace=MEM_DEVICE, stream=0):
        """eqlb_mesh_lagrange_dofmap on a raw pointer [ncells, nd_p] int32 in `memspace`; returns ndofs."""
        n = C.c_int64(0)
        _check(lib().eqlb_mesh_lagrange_dofmap(self._h, C.c_int32(p), _vp(cell_dofs), C.byref(n), C.c_int32(memspace),
                                               C.c_void_p(stream)))
        return int(n.value)

    def lagrange_dofmap(self, p, device=False, stream=0):
        """(cell_dofs [ncells, nd_p] int32, ndofs) of the conforming P_p space, 1 <= p <= 4, in the numbering of
        mesh.transfer.lagrange_dofmap (eqlb_mesh_lagrange_dofmap): what primal_flux_dg and Refinement.prolong take on
        a handle that has no dofmap of the caller's.  device=True: a torch tensor on the device, written on `stream`."""
        nd = (max(int(p), 0) + 1) * (max(int(p), 0) + 2) // 2
        nc = self.counts()[1]
        if device:
            import torch
            cd = torch.empty((nc, nd), dtype=torch.int32, device="cuda")
            return cd, self.lagrange_dofmap_raw(p, cd.data_ptr(), MEM_DEVICE, stream)
        cd = np.zeros((nc, nd), dtype=np.int32)
        return cd, self.lagrange_dofmap_raw(p, cd.ctypes.data, MEM_HOST, stream)

    def refine_raw(self, marked, nmarked, capacity, memspace=MEM_DEVICE, stream=0):
        """eqlb_mesh_refine_plan on raw pointers (ints) in `memspace`: the marked list and its int64 length exactly as
        mark_doerfler_raw leaves them.  Returns a RefinePlan; this mesh must outlive it."""
        return RefinePlan(self, marked, nmarked, capacity, memspace, stream)

    def refine(self, marked, device=False, stream=0, keep_plan=False):
        """The mesh refined at the cells `marked` by longest-edge closure and bisection, on the device
        (eqlb_mesh_refine_plan ...; the rule: mesh.refine.refine_longest_edge).  Returns a Refinement: `.dmesh` (the new
        DeviceMesh, `.mesh` filled as from_cells does), `.parent_cell`, `.node_parent_facet`, `.parent_facet`, `.counts`.
        device=False: `marked` is a host array of cell ids.  device=True: `marked` is a pair (ids, count) of torch
        tensors on the device (int32 [capacity], int64 [1]) as mark_doerfler_raw leaves them, read on `stream`; the
        parent arrays come back as device tensors.
        keep_plan=True keeps the plan open on the Refinement (`.plan`), so that Refinement.prolong / prolong_dg can
        carry solutions and DG data over; Refinement.close() releases it.  This mesh must outlive it."""
        from .mesh import Mesh
        if device:
            import torch
            ids, count = marked
            if ids.element_size() != 4 or count.element_size() != 8 or not ids.is_contiguous():
                raise RuntimeError("DeviceMesh.refine: contiguous int32 ids and an int64 count expected")
            plan = self.refine_raw(ids.data_ptr(), count.data_ptr(), int(ids.numel()), MEM_DEVICE, stream)
        else:
            ids = np.ascontiguousarray(marked, dtype=np.int32).ravel()
            count = np.array([ids.size], dtype=np.int64)
            plan = self.refine_raw(ids.ctypes.data, count.ctypes.data, ids.size, MEM_HOST, stream)
        try:
            nn2, nc2, nbis, ncut = plan.counts()
            hx = np.zeros((nn2, 3))
            hc = np.zeros((nc2, 3), dtype=np.int32)
            dm = plan.create_mesh(stream)
            nf2 = dm.counts()[2]
            if device:
                pc, npf, pf = [torch.empty(n, dtype=torch.int32, device=ids.device) for n in (nc2, nbis, nf2)]
                plan.write_raw(None, None, pc.data_ptr(), npf.data_ptr(), MEM_DEVICE, stream)
                plan.parent_facets_raw(dm, pf.data_ptr(), MEM_DEVICE, stream)
                plan.write_raw(hx.ctypes.data, hc.ctypes.data, None, None, MEM_HOST, stream)   # (waits for `stream`)
            else:
                pc, npf, pf = [np.zeros(n, dtype=np.int32) for n in (nc2, nbis, nf2)]
                plan.write_raw(hx.ctypes.data, hc.ctypes.data, pc.ctypes.data, npf.ctypes.data, MEM_HOST, stream)
                plan.parent_facets_raw(dm, pf.ctypes.data, MEM_HOST, stream)
        except BaseException:
            plan.close()
            raise
        if not keep_plan:
            plan.close()
        t = dm.export()
        dm.mesh = Mesh(hx, hc, t["cell_facets"], t["facet_nodes"], t["facet_cells_offsets"], t["facet_cells"],
                       t["node_cells_offsets"], t["node_cells"], t["node_facets_offsets"], t["node_facets"],
                       t["facet_perm"])
        return Refinement(dm, pc, npf, pf, {"nnodes2": nn2, "ncells2": nc2, "nbisected": nbis, "ncells_cut": ncut},
                          plan if keep_plan else None)

    @property
    def max_patch_cells(self):
        return int(lib().eqlb_mesh_max_patch_cells(self._h))

    def close(self):
        if self._h:
            lib().eqlb_mesh_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RefinePlan:
    """eqlb_refine_t: closure and scans of a refinement, kept on the device (DeviceMesh.refine_raw)."""

    def __init__(self, dmesh, marked, nmarked, capacity, memspace, stream):
        self.dmesh = dmesh   # the plan reads the handle: keep it alive
        self._h = C.c_void_p()
        _check(lib().eqlb_mesh_refine_plan(dmesh._h, _vp(marked), _vp(nmarked), C.c_int64(capacity),
                                           C.c_int32(memspace), C.c_void_p(stream), C.byref(self._h)))

    def counts(self):
        """(nnodes2, ncells2, nbisected, ncells_cut) (eqlb_refine_counts)."""
        v = [C.c_int32(0) for _ in range(4)]
        _check(lib().eqlb_refine_counts(self._h, *[C.byref(a) for a in v]))
        return tuple(int(a.value) for a in v)

    def write_raw(self, x2, cell_nodes2, parent_cell, node_parent_facet, memspace=MEM_DEVICE, stream=0):
        """eqlb_refine_write on raw pointers (ints, None for an output that is not wanted) in `memspace`."""
        _check(lib().eqlb_refine_write(self._h, _vp(x2), _vp(cell_nodes2), _vp(parent_cell), _vp(node_parent_facet),
                                       C.c_int32(memspace), C.c_void_p(stream)))

    def create_mesh(self, stream=0):
        """eqlb_refine_create_mesh: the DeviceMesh of the refined mesh (`.mesh` is not filled)."""
        dm = DeviceMesh.__new__(DeviceMesh)
        dm._h = C.c_void_p()
        dm.mesh = None
        _check(lib().eqlb_refine_create_mesh(self._h, C.c_void_p(stream), C.byref(dm._h)))
        return dm

    def parent_facets_raw(self, refined, parent_facet, memspace=MEM_DEVICE, stream=0):
        """eqlb_refine_parent_facets on a raw pointer [nfacets of `refined`] in `memspace`."""
        _check(lib().eqlb_refine_parent_facets(self._h, refined._h, _vp(parent_facet), C.c_int32(memspace),
                                               C.c_void_p(stream)))

    def prolong_lagrange_raw(self, refined, p, bs, nrhs, cell_dofs, ndofs, u, cell_dofs2, ndofs2, u2,
                             memspace=MEM_DEVICE, stream=0):
        """eqlb_refine_prolong_lagrange on raw pointers (ints) in `memspace`: u [nrhs, ndofs*bs] of the P_p space on
        the mesh of the plan -> u2 [nrhs, ndofs2*bs] on `refined`, through the caller's dofmaps."""
        _check(lib().eqlb_refine_prolong_lagrange(self._h, refined._h, C.c_int32(p), C.c_int32(bs), C.c_int32(nrhs),
                                                  _vp(cell_dofs), C.c_int64(ndofs), _vp(u), _vp(cell_dofs2),
                                                  C.c_int64(ndofs2), _vp(u2), C.c_int32(memspace), C.c_void_p(stream)))

    def prolong_dg_raw(self, refined, degree, bs, nrhs, values, out, memspace=MEM_DEVICE, stream=0):
        """eqlb_refine_prolong_dg on raw pointers (ints) in `memspace`: [nrhs, ncells*nd*bs] -> [nrhs, ncells2*nd*bs]."""
        _check(lib().eqlb_refine_prolong_dg(self._h, refined._h, C.c_int32(degree), C.c_int32(bs), C.c_int32(nrhs),
                                            _vp(values), _vp(out), C.c_int32(memspace), C.c_void_p(stream)))

    def facet_types_raw(self, refined, nrhs, facet_type, facet_type2, memspace=MEM_DEVICE, stream=0):
        """eqlb_refine_facet_types on raw pointers (ints) in `memspace`: int8 [nrhs, nfacets] -> [nrhs, nfacets2]."""
        _check(lib().eqlb_refine_facet_types(self._h, refined._h, C.c_int32(nrhs), _vp(facet_type), _vp(facet_type2),
                                             C.c_int32(memspace), C.c_void_p(stream)))

    def child_facets_raw(self, refined, nlist, facets, children, memspace=MEM_DEVICE, stream=0):
        """eqlb_refine_child_facets on raw pointers (ints) in `memspace`: old ids [nlist] -> children [nlist, 2]."""
        _check(lib().eqlb_refine_child_facets(self._h, refined._h, C.c_int32(nlist), _vp(facets), _vp(children),
                                              C.c_int32(memspace), C.c_void_p(stream)))

    def prolong_flux_bc_raw(self, refined, k, nrhs, boundary_values, nlist, facets2, dofs, memspace=MEM_DEVICE,
                            stream=0):
        """eqlb_refine_prolong_flux_bc on raw pointers (ints) in `memspace`: the table [nrhs, ncells*k(k+2)] of the old
        mesh -> dofs [nrhs, nlist, k] of the listed boundary facets of `refined`."""
        _check(lib().eqlb_refine_prolong_flux_bc(self._h, refined._h, C.c_int32(k), C.c_int32(nrhs),
                                                 _vp(boundary_values), C.c_int32(nlist), _vp(facets2), _vp(dofs),
                                                 C.c_int32(memspace), C.c_void_p(stream)))

    def close(self):
        if self._h:
            lib().eqlb_refine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Refinement:
    """Result of DeviceMesh.refine: the refined DeviceMesh and the parent tables (host arrays or device tensors)."""

    def __init__(self, dmesh, parent_cell, node_parent_facet, parent_facet, counts, plan=None):
        self.dmesh = dmesh
        self.parent_cell = parent_cell
        self.node_parent_facet = node_parent_facet
        self.parent_facet = parent_facet
        self.counts = counts
        self.plan = plan   # the open RefinePlan of DeviceMesh.refine(..., keep_plan=True), else None

    def _kept_plan(self, who):
        if self.plan is None or not self.plan._h:
            raise RuntimeError(f"Refinement.{who}: the plan of the refinement was not kept "
                               "(DeviceMesh.refine(..., keep_plan=True)) or is closed")
        return self.plan

    def prolong(self, p, u, cell_dofs=None, cell_dofs2=None, bs=1, ndofs2=None, out=None, stream=0):
        """u [nrhs, ndofs*bs] (or [ndofs*bs]) in P_p on the old mesh -> [nrhs, ndofs2*bs] on the refined mesh
        (eqlb_refine_prolong_lagrange; the rule: mesh.transfer.prolong_lagrange).  Host arrays, or torch tensors on the
        device, which are read and written on `stream`.  cell_dofs / cell_dofs2: the caller's dofmaps, None:
        lagrange_dofmap of the two handles; ndofs2: size of the new space (None: that of lagrange_dofmap, or max + 1
        of a host cell_dofs2 - required with a caller's dofmap on the device).  Every DOF of cell_dofs2 is written,
        the other entries keep what `out` holds (None: zeros)."""
        plan = self._kept_plan("prolong")
        dev = hasattr(u, "data_ptr")
        nd = (p + 1) * (p + 2) // 2
        if cell_dofs is None:
            cell_dofs, _ = plan.dmesh.lagrange_dofmap(p, device=dev, stream=stream)
        if cell_dofs2 is None:
            cell_dofs2, ndofs2 = self.dmesh.lagrange_dofmap(p, device=dev, stream=stream)
        if dev:
            import torch
            if ndofs2 is None:
                raise RuntimeError("Refinement.prolong: ndofs2 is needed with a caller's cell_dofs2 on the device")
            if not (u.is_contiguous() and cell_dofs.is_contiguous() and cell_dofs2.is_contiguous()) \
                    or u.element_size() != 8 or cell_dofs.element_size() != 4 or cell_dofs2.element_size() != 4:
                raise RuntimeError("Refinement.prolong: contiguous float64 u and int32 dofmaps expected")
            uu = u.reshape(1, -1) if u.dim() == 1 else u
            if out is None:   # the zero fill goes on `stream`, in front of the kernel; nothing waits
                fill = torch.cuda.ExternalStream(stream) if stream else torch.cuda.default_stream(u.device)
                with torch.cuda.stream(fill):
                    out = torch.zeros((uu.shape[0], int(ndofs2) * bs), dtype=torch.float64, device=u.device)
            ptrs = (cell_dofs.data_ptr(), uu.data_ptr(), cell_dofs2.data_ptr(), out.data_ptr())
            ncd, ncd2, nu, nout = cell_dofs.numel(), cell_dofs2.numel(), uu.shape[1], out.numel()
            memspace = MEM_DEVICE
        else:
            uu = np.ascontiguousarray(u, dtype=np.float64)
            uu = uu.reshape(1, -1) if uu.ndim == 1 else uu
            cell_dofs = np.ascontiguousarray(cell_dofs, dtype=np.int32)
            cell_dofs2 = np.ascontiguousarray(cell_dofs2, dtype=np.int32)
            if ndofs2 is None:
                ndofs2 = int(cell_dofs2.max()) + 1
            if out is None:
                out = np.zeros((uu.shape[0], int(ndofs2) * bs))
            assert out.dtype == np.float64 and out.flags.c_contiguous
            ptrs = (cell_dofs.ctypes.data, uu.ctypes.data, cell_dofs2.ctypes.data, out.ctypes.data)
            ncd, ncd2, nu, nout = cell_dofs.size, cell_dofs2.size, uu.shape[1], out.size
            memspace = MEM_HOST
        nrhs = int(uu.shape[0])
        nc, nc2 = plan.dmesh.counts()[1], self.counts["ncells2"]
        if nu % bs != 0 or ncd != nc * nd or ncd2 != nc2 * nd or nout != nrhs * int(ndofs2) * bs:
            raise RuntimeError("Refinement.prolong: Input sizes does not match")
        plan.prolong_lagrange_raw(self.dmesh, p, bs, nrhs, ptrs[0], nu // bs, ptrs[1], ptrs[2], int(ndofs2), ptrs[3],
                                  memspace, stream)
        return out[0] if len(u.shape) == 1 and len(out.shape) == 2 else out

    def prolong_dg(self, degree, values, bs=1, stream=0):
        """values [nrhs, ncells*nd*bs] (or 1-D) of DG_degree data on the old mesh -> [nrhs, ncells2*nd*bs] on the
        refined mesh (eqlb_refine_prolong_dg): flux_dg with bs = 2, rhs_dg with bs = 1, a cell-wise coefficient with
        degree = 0.  Host arrays, or torch tensors on the device, read and written on `stream`."""
        plan = self._kept_plan("prolong_dg")
        nd = (degree + 1) * (degree + 2) // 2
        nc, nc2 = plan.dmesh.counts()[1], self.counts["ncells2"]
        dev = hasattr(values, "data_ptr")
        if dev:
            import torch
            if not values.is_contiguous() or values.element_size() != 8:
                raise RuntimeError("Refinement.prolong_dg: contiguous float64 values expected")
            v = values.reshape(1, -1) if values.dim() == 1 else values
            out = torch.empty((v.shape[0], nc2 * nd * bs), dtype=torch.float64, device=values.device)
            pin, pout, memspace = v.data_ptr(), out.data_ptr(), MEM_DEVICE
        else:
            v = np.ascontiguousarray(values, dtype=np.float64)
            v = v.reshape(1, -1) if v.ndim == 1 else v
            out = np.zeros((v.shape[0], nc2 * nd * bs))
            pin, pout, memspace = v.ctypes.data, out.ctypes.data, MEM_HOST
        if nd < 1 or v.shape[1] != nc * nd * bs:
            raise RuntimeError("Refinement.prolong_dg: Input sizes does not match")
        plan.prolong_dg_raw(self.dmesh, degree, bs, int(v.shape[0]), pin, pout, memspace, stream)
        return out[0] if len(values.shape) == 1 else out

    def facet_types(self, facet_type, stream=0):
        """facet_type [nrhs, nfacets] (or 1-D) int8 of the old mesh -> [nrhs, nfacets2] of the refined mesh: the type
        of the parent facet, EQLB_FACET_INTERNAL where there is none (eqlb_refine_facet_types; the rule:
        mesh.refine.carry_facet_types).  Host arrays, or torch tensors on the device, read and written on `stream`."""
        plan = self._kept_plan("facet_types")
        nf, nf2 = plan.dmesh.counts()[2], self.dmesh.counts()[2]
        if hasattr(facet_type, "data_ptr"):
            import torch
            if not facet_type.is_contiguous() or facet_type.element_size() != 1:
                raise RuntimeError("Refinement.facet_types: contiguous int8 types expected")
            ft = facet_type.reshape(1, -1) if facet_type.dim() == 1 else facet_type
            out = torch.empty((ft.shape[0], nf2), dtype=torch.int8, device=facet_type.device)
            pin, pout, memspace = ft.data_ptr(), out.data_ptr(), MEM_DEVICE
        else:
            ft = np.ascontiguousarray(facet_type, dtype=np.int8)
            ft = ft.reshape(1, -1) if ft.ndim == 1 else ft
            out = np.zeros((ft.shape[0], nf2), dtype=np.int8)
            pin, pout, memspace = ft.ctypes.data, out.ctypes.data, MEM_HOST
        if ft.shape[1] != nf:
            raise RuntimeError("Refinement.facet_types: Input sizes does not match")
        plan.facet_types_raw(self.dmesh, int(ft.shape[0]), pin, pout, memspace, stream)
        return out[0] if len(facet_type.shape) == 1 else out

    def child_facets(self, facets, flat=False, stream=0):
        """children [nlist, 2] int32 of the old facets `facets` in the numbering of the refined mesh, (f2, -1) for a
        facet that is not bisected (eqlb_refine_child_facets; the rule: mesh.refine.child_facets) - the inverse of
        `.parent_facet` for the facets of a flux boundary condition, a Dirichlet list, facet tags.  flat=True (host
        arrays): the list of the children without the -1 entries, in the order of `facets`.  Host arrays, or torch
        tensors on the device, read and written on `stream`."""
        plan = self._kept_plan("child_facets")
        if hasattr(facets, "data_ptr"):
            import torch
            if flat:
                raise RuntimeError("Refinement.child_facets: flat=True needs host arrays")
            if not facets.is_contiguous() or facets.element_size() != 4:
                raise RuntimeError("Refinement.child_facets: contiguous int32 ids expected")
            out = torch.empty((facets.numel(), 2), dtype=torch.int32, device=facets.device)
            plan.child_facets_raw(self.dmesh, int(facets.numel()), facets.data_ptr(), out.data_ptr(), MEM_DEVICE,
                                  stream)
            return out
        fl = np.ascontiguousarray(facets, dtype=np.int32).ravel()
        out = np.zeros((fl.size, 2), dtype=np.int32)
        plan.child_facets_raw(self.dmesh, fl.size, fl.ctypes.data, out.ctypes.data, MEM_HOST, stream)
        return out[out >= 0] if flat else out

    def _carry_facet_term(self, old, new, stream):
        """The list of the facet term of `old` (its _facet names the term) through child_facets - in the order of the
        list, first child first, a child takes its parent's values - into the host setter of `new`."""
        f, v = old._facet_list()
        ch = self.child_facets(f, stream=stream)
        keep = ch >= 0
        f2 = ch[keep].astype(np.int32)
        v2 = np.repeat(v[:, None], 2, axis=1)[keep]
        new._facet_set(f2, [1.0], v2, stream)   # (the scalar at its default: the values are given per facet)
        return f2, v2

    def carry_robin(self, old, new, stream=0):
        """The Robin list of the solver handle `old` (PrimalPoisson on the mesh that was refined) on the refined mesh:
        the list goes through child_facets, a child takes its parent's alpha, and `new` (PrimalPoisson on the refined
        mesh) gets it through set_robin (the rule: mesh.refine.carry_robin_list).  Returns (facets2, facet_alpha2), host
        arrays.  `old` must have received its list through set_robin (host arrays) - one whose list came through
        set_robin_raw is refused, and `new` stays as it was; one without the term switches the term of `new` off."""
        return self._carry_facet_term(old, new, stream)

    def carry_springs(self, old, new, stream=0):
        """The spring list of the solver handle `old` (PrimalElasticity on the mesh that was refined) on the refined
        mesh: the list goes through child_facets, a child takes its parent's tensor K as it is - K is stated in global
        axes, so nothing is rotated - and `new` (PrimalElasticity on the refined mesh) gets it through set_springs (the
        rule: mesh.refine.carry_springs_list).  Returns (facets2, facet_k2), host arrays.  `old` must have received its
        list through set_springs (host arrays); one without the term switches the term of `new` off."""
        return self._carry_facet_term(old, new, stream)

    def prolong_flux_bc(self, k, boundary_values, facets2, stream=0):
        """The table boundary_values [nrhs, ncells*k(k+2)] (or 1-D) of the old mesh -> dofs [nrhs, nlist, k] of the
        boundary facets `facets2` of the refined mesh, each row as update_flux_bc takes it without a rule
        (eqlb_refine_prolong_flux_bc; the rule: mesh.transfer.prolong_flux_bc).  Host arrays, or torch tensors on the
        device, read and written on `stream`."""
        plan = self._kept_plan("prolong_flux_bc")
        nc = plan.dmesh.counts()[1]
        ntab = nc * max(int(k), 0) * (max(int(k), 0) + 2)
        if hasattr(boundary_values, "data_ptr"):
            import torch
            if not (boundary_values.is_contiguous() and facets2.is_contiguous()) \
                    or boundary_values.element_size() != 8 or facets2.element_size() != 4:
                raise RuntimeError("Refinement.prolong_flux_bc: contiguous float64 values and int32 ids expected")
            bv = boundary_values.reshape(1, -1) if boundary_values.dim() == 1 else boundary_values
            nlist = int(facets2.numel())
            out = torch.empty((bv.shape[0], nlist, max(int(k), 0)), dtype=torch.float64, device=bv.device)
            ptrs, memspace = (bv.data_ptr(), facets2.data_ptr(), out.data_ptr()), MEM_DEVICE
        else:
            bv = np.ascontiguousarray(boundary_values, dtype=np.float64)
            bv = bv.reshape(1, -1) if bv.ndim == 1 else bv
            fl = np.ascontiguousarray(facets2, dtype=np.int32).ravel()
            nlist = fl.size
            out = np.zeros((bv.shape[0], nlist, max(int(k), 0)))
            ptrs, memspace = (bv.ctypes.data, fl.ctypes.data, out.ctypes.data), MEM_HOST
        if ntab > 0 and bv.shape[1] != ntab:
            raise RuntimeError("Refinement.prolong_flux_bc: Input sizes does not match")
        plan.prolong_flux_bc_raw(self.dmesh, k, int(bv.shape[0]), ptrs[0], nlist, ptrs[1], ptrs[2], memspace, stream)
        return out[0] if len(boundary_values.shape) == 1 else out

    def close(self):
        """Releases the kept plan (the refined DeviceMesh stays)."""
        if self.plan is not None:
            self.plan.close()
            self.plan = None


class SemiExplicitEquilibrator:
    """eqlb_se_* handle: RT_k equilibrator on a device mesh."""

    def __init__(self, dmesh: DeviceMesh, k: int, nrhs: int, degree_dg=None,
                 reconstruct_stress=False, estimate_korn=False):
        self.dmesh = dmesh
        self.k, self.nrhs = k, nrhs
        self.reconstruct_stress = bool(reconstruct_stress)
        self.degree_dg = k - 1 if degree_dg is None else degree_dg
        self.nrt = k * (k + 2)
        self.nd = (self.degree_dg + 1) * (self.degree_dg + 2) // 2
        self._h = C.c_void_p()
        _check(lib().eqlb_se_create(dmesh._h, C.c_int32(k), C.c_int32(self.degree_dg),
                                    C.c_int32(nrhs), C.c_int32(int(reconstruct_stress)),
                                    C.c_int32(int(estimate_korn)), C.byref(self._h)))

    def set_option(self, key: str, value: int):
        _check(lib().eqlb_se_set_option(self._h, key.encode(), C.c_int32(value)))

    def set_boundary(self, facet_type, boundary_values=None, node_mask=None):
        m = self.dmesh.mesh
        ft = np.ascontiguousarray(facet_type, dtype=np.int8).reshape(self.nrhs, m.nfacets)
        bv = None
        if boundary_values is not None:
            bv = np.ascontiguousarray(boundary_values, dtype=np.float64)
            assert bv.size == self.nrhs * m.ncells * self.nrt
        nm = None
        if node_mask is not None:
            nm = np.ascontiguousarray(node_mask, dtype=np.uint8)
            assert nm.size == m.nnodes
        _check(lib().eqlb_se_set_boundary(self._h, _hp(ft), _hp(bv) if bv is not None else None,
                                          _hp(nm) if nm is not None else None))

    def update_flux_bc(self, rhs: int, facets, values, s=None, w=None, vector=False):
        """eqlb_se_update_flux_bc on host arrays: new boundary values of right-hand side `rhs` on the listed
        flux-BC facets, nothing else of the handle changes.  values [nlist, k] facet DOFs as flux_bc_dofs returns
        them (s is None), or point values at the rule (s, w): [nlist, nq] normal flux, [nlist, nq, 2] with vector."""
        _update_flux_bc(lib().eqlb_se_update_flux_bc, self, rhs, facets, values, s, w, vector)

    def update_flux_bc_raw(self, rhs: int, nlist: int, facets, values, s=None, w=None, vector=False, nrejected=None,
                           memspace=MEM_DEVICE, stream=0):
        """eqlb_se_update_flux_bc on raw pointers (ints) in `memspace`, ordered on `stream`; s, w stay host arrays.
        Device memory: one kernel, nothing waits; nrejected [1] int32 (or None) counts the refused entries."""
        _update_flux_bc_raw(lib().eqlb_se_update_flux_bc, self, rhs, nlist, facets, values, s, w, vector, nrejected,
                            memspace, stream)

    def carry_boundary(self, old, refinement, node_mask=None, stream=0):
        """eqlb_se_carry_boundary: the boundary conditions of `old` (a SemiExplicitEquilibrator on the coarse mesh with
        an accepted set_boundary) set on this handle, which lives on `refinement.dmesh`; `refinement` keeps its plan
        (DeviceMesh.refine(..., keep_plan=True)).  The facet types are gathered on the device and planned as
        set_boundary plans them; a value table of `old` is carried from table to table on the device."""
        _carry_boundary(lib().eqlb_se_carry_boundary, self, old, refinement, node_mask, stream)

    def get_boundary_values(self):
        """eqlb_se_get_boundary_values: the table [nrhs, ncells*k(k+2)] of the handle (zeros if homogeneous)."""
        return _get_boundary_values(lib().eqlb_se_get_boundary_values, self)

    def get_boundary_values_raw(self, out, memspace=MEM_DEVICE, stream=0):
        _check(lib().eqlb_se_get_boundary_values(self._h, _vp(out), C.c_int32(memspace), C.c_void_p(stream)))

    @property
    def num_patches(self):
        return int(lib().eqlb_se_num_patches(self._h))

    def tiling_info(self):
        """dict(ntiles, cells_per_tile, patch_instances, lane_slots) of the tiled launch."""
        v = [C.c_int64(0) for _ in range(4)]
        _check(lib().eqlb_se_tiling_info(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("ntiles", "cells_per_tile", "patch_instances", "lane_slots"),
                        [int(x.value) for x in v]))

    def tiling_blocks(self):
        """Wave-blocks of the tiled launch per body instance and bin (eqlb_se_tiling_blocks): dict kind ->
        [count for P = 4, 8, 16, 32, 64] for the kinds of TILING_BLOCK_KINDS, and "zero_tiles"."""
        return _tiling_blocks(lib().eqlb_se_tiling_blocks, self._h)

    def large_patch_info(self):
        """(npatches, max_cells) of the patches with more than 63 cells or 64 facets that the last set_boundary
        handed to the large-patch kernel (option "large_patches"; eqlb_se_large_patch_info)."""
        return _large_patch_info(lib().eqlb_se_large_patch_info, self._h)

    def equilibrate_host(self, flux_dg, rhs_dg, flux_hdiv=None):
        """Host numpy arrays in/out; flux_hdiv is accumulated (+=) like the reference."""
        m = self.dmesh.mesh
        g = np.ascontiguousarray(flux_dg, dtype=np.float64).reshape(self.nrhs, -1)
        f = np.ascontiguousarray(rhs_dg, dtype=np.float64).reshape(self.nrhs, -1)
        if g.shape[1] != m.ncells * self.nd * 2 or f.shape[1] != m.ncells * self.nd:
            raise RuntimeError("Equilibration: Input sizes does not match")
        if flux_hdiv is None:
            flux_hdiv = np.zeros((self.nrhs, m.ncells * self.nrt))
        assert flux_hdiv.dtype == np.float64 and flux_hdiv.flags.c_contiguous
        assert flux_hdiv.size == self.nrhs * m.ncells * self.nrt
        _check(lib().eqlb_se_equilibrate(self._h, _hp(g), _hp(f), _hp(flux_hdiv),
                                         C.c_int32(MEM_HOST), None))
        return flux_hdiv

    def equilibrate_host_with_kornconst(self, flux_dg, rhs_dg, flux_hdiv=None, korn=None):
        """As equilibrate_host, plus the accumulated squared Korn constants [ncells]."""
        m = self.dmesh.mesh
        g = np.ascontiguousarray(flux_dg, dtype=np.float64).reshape(self.nrhs, -1)
        f = np.ascontiguousarray(rhs_dg, dtype=np.float64).reshape(self.nrhs, -1)
        if g.shape[1] != m.ncells * self.nd * 2 or f.shape[1] != m.ncells * self.nd:
            raise RuntimeError("Equilibration: Input sizes does not match")
        if flux_hdiv is None:
            flux_hdiv = np.zeros((self.nrhs, m.ncells * self.nrt))
        if korn is None:
            korn = np.zeros(m.ncells)
        _check(lib().eqlb_se_equilibrate_with_kornconst(self._h, _hp(g), _hp(f), _hp(flux_hdiv),
                                                        _hp(korn), C.c_int32(MEM_HOST), None))
        return flux_hdiv, korn

    def kornconst_host(self, korn=None):
        """eqlb_se_kornconst: the squared Korn constants of the patches added to korn [ncells] (host memory)."""
        m = self.dmesh.mesh
        if korn is None:
            korn = np.zeros(m.ncells)
        assert korn.dtype == np.float64 and korn.flags.c_contiguous and korn.size == m.ncells
        _check(lib().eqlb_se_kornconst(self._h, _hp(korn), C.c_int32(MEM_HOST), None))
        return korn

    def equilibrate_device(self, flux_dg_ptr: int, rhs_dg_ptr: int, flux_hdiv_ptr: int,
                           stream: int = 0):
        """Raw device pointers (e.g. torch tensor .data_ptr()) and a hipStream_t handle;
        asynchronous."""
        _check(lib().eqlb_se_equilibrate(self._h, C.c_void_p(flux_dg_ptr), C.c_void_p(rhs_dg_ptr),
                                         C.c_void_p(flux_hdiv_ptr), C.c_int32(MEM_DEVICE),
                                         C.c_void_p(stream)))

    def equilibrate_device_tiles(self, flux_dg_ptr: int, rhs_dg_ptr: int, flux_hdiv_ptr: int,
                                 tile_first: int, tile_count: int, stream: int = 0):
        """equilibrate_device for a range of tiles (tiled scatter; count -1 = to the end)."""
        _check(lib().eqlb_se_equilibrate_tiles(self._h, C.c_void_p(flux_dg_ptr), C.c_void_p(rhs_dg_ptr),
                                               C.c_void_p(flux_hdiv_ptr), C.c_int32(tile_first),
                                               C.c_int32(tile_count), C.c_void_p(stream)))

    def set_priority_cells(self, cells):
        """Cells whose tiles become the first tiles at the next set_boundary (two-phase sweeps)."""
        c = np.ascontiguousarray(cells, dtype=np.int32)
        _check(lib().eqlb_se_set_priority_cells(self._h, _hp(c), C.c_int32(c.size)))

    @property
    def num_priority_tiles(self) -> int:
        return int(lib().eqlb_se_num_priority_tiles(self._h))

    def check_status(self, stream: int = 0):
        """After device-memory calls: waits for the stream and raises if a patch system was not
        positive definite (degenerate cell geometry)."""
        _check(lib().eqlb_se_check_status(self._h, C.c_void_p(stream)))

    def last_kernel_ms(self, which=0):
        return float(lib().eqlb_se_last_kernel_ms(self._h, C.c_int32(which)))

    def export_patches(self):
        m = self.dmesh.mesh
        stride = self.dmesh.max_patch_cells + 2
        nn = m.nnodes
        out = dict(ncells=np.zeros(nn, np.int32), cells=np.zeros((nn, stride), np.int32),
                   fcts=np.zeros((nn, stride), np.int32),
                   fcts_local=np.zeros((nn, 2 * stride), np.int8),
                   inodes_local=np.zeros((nn, stride), np.int8),
                   reversed=np.zeros((nn, 2 * stride), np.int8), stride=stride)
        _check(lib().eqlb_se_export_patches(self._h, C.c_int32(stride), _hp(out["ncells"]),
                                            _hp(out["cells"]), _hp(out["fcts"]),
                                            _hp(out["fcts_local"]), _hp(out["inodes_local"]),
                                            _hp(out["reversed"])))
        return out

    def close(self):
        if self._h:
            lib().eqlb_se_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ConstrainedMinEquilibrator:
    """eqlb_ev_* handle: constrained-minimisation (Ern-Vohralik) equilibrator, flux in the
    conforming hierarchic RT_k (include/eqlb.h)."""

    def __init__(self, dmesh: DeviceMesh, k: int, nrhs: int, cell_dofs=None, ndofs=None, degree_dg=None):
        self.dmesh = dmesh
        self.k, self.nrhs = k, nrhs
        self.degree_dg = k - 1 if degree_dg is None else degree_dg
        self.nrt = k * (k + 2)
        self.nd = (self.degree_dg + 1) * (self.degree_dg + 2) // 2
        self.output = 0
        self._h = C.c_void_p()
        _check(lib().eqlb_ev_create_dg(dmesh._h, C.c_int32(k), C.c_int32(self.degree_dg), C.c_int32(nrhs),
                                       C.byref(self._h)))
        if cell_dofs is not None:
            cd = np.ascontiguousarray(cell_dofs, dtype=np.int32)
            assert cd.shape == (dmesh.mesh.ncells, self.nrt)
            _check(lib().eqlb_ev_set_dofmap(self._h, _hp(cd), C.c_int64(int(ndofs))))

    def set_basis_transform(self, C=None, R=None):
        """Change of basis of the conforming output (eqlb_ev_set_basis_transform): C [nrt, nrt], R [k, k]."""
        c = None if C is None else np.ascontiguousarray(C, dtype=np.float64)
        r = None if R is None else np.ascontiguousarray(R, dtype=np.float64)
        if c is not None:
            assert c.shape == (self.nrt, self.nrt) and (r is None or r.shape == (self.k, self.k))
        _check(lib().eqlb_ev_set_basis_transform(self._h, _hp(c) if c is not None else None,
                                                 _hp(r) if r is not None else None))

    @property
    def ndofs(self):
        return int(lib().eqlb_ev_num_dofs(self._h))

    @property
    def num_patches(self):
        return int(lib().eqlb_ev_num_patches(self._h))

    def set_option(self, key: str, value: int):
        _check(lib().eqlb_ev_set_option(self._h, key.encode(), C.c_int32(value)))
        if key == "output":
            self.output = value

    def set_boundary(self, facet_type, boundary_values=None, node_mask=None):
        m = self.dmesh.mesh
        ft = np.ascontiguousarray(facet_type, dtype=np.int8).reshape(self.nrhs, m.nfacets)
        bv = None
        if boundary_values is not None:
            bv = np.ascontiguousarray(boundary_values, dtype=np.float64)
            assert bv.size == self.nrhs * self.ndofs
        nm = None
        if node_mask is not None:
            nm = np.ascontiguousarray(node_mask, dtype=np.uint8)
            assert nm.size == m.nnodes
        _check(lib().eqlb_ev_set_boundary(self._h, _hp(ft), _hp(bv) if bv is not None else None,
                                          _hp(nm) if nm is not None else None))

    def update_flux_bc(self, rhs: int, facets, values, s=None, w=None, vector=False):
        """eqlb_ev_update_flux_bc on host arrays: new boundary values of right-hand side `rhs` on the listed
        flux-BC facets, nothing else of the handle changes; the values
        are moments in the frame of the facet's cell whatever the output basis is.  values [nlist, k] facet DOFs as flux_bc_dofs returns
        them (s is None), or point values at the rule (s, w): [nlist, nq] normal flux, [nlist, nq, 2] with vector."""
        _update_flux_bc(lib().eqlb_ev_update_flux_bc, self, rhs, facets, values, s, w, vector)

    def update_flux_bc_raw(self, rhs: int, nlist: int, facets, values, s=None, w=None, vector=False, nrejected=None,
                           memspace=MEM_DEVICE, stream=0):
        """eqlb_ev_update_flux_bc on raw pointers (ints) in `memspace`, ordered on `stream`; s, w stay host arrays.
        Device memory: one kernel, nothing waits; nrejected [1] int32 (or None) counts the refused entries."""
        _update_flux_bc_raw(lib().eqlb_ev_update_flux_bc, self, rhs, nlist, facets, values, s, w, vector, nrejected,
                            memspace, stream)

    def carry_boundary(self, old, refinement, node_mask=None, stream=0):
        """eqlb_ev_carry_boundary: as SemiExplicitEquilibrator.carry_boundary, on the broken per-cell table of the EV
        handle; the dofmap and the basis transform of this handle are set first, as before set_boundary."""
        _carry_boundary(lib().eqlb_ev_carry_boundary, self, old, refinement, node_mask, stream)

    def get_boundary_values(self):
        """eqlb_ev_get_boundary_values: the table [nrhs, ncells*k(k+2)] of the handle in the broken per-cell
        layout (zeros if homogeneous)."""
        return _get_boundary_values(lib().eqlb_ev_get_boundary_values, self)

    def get_boundary_values_raw(self, out, memspace=MEM_DEVICE, stream=0):
        _check(lib().eqlb_ev_get_boundary_values(self._h, _vp(out), C.c_int32(memspace), C.c_void_p(stream)))

    def tiling_blocks(self):
        """As SemiExplicitEquilibrator.tiling_blocks (eqlb_ev_tiling_blocks)."""
        return _tiling_blocks(lib().eqlb_ev_tiling_blocks, self._h)

    def large_patch_info(self):
        """As SemiExplicitEquilibrator.large_patch_info (eqlb_ev_large_patch_info)."""
        return _large_patch_info(lib().eqlb_ev_large_patch_info, self._h)

    def _nout(self):
        return self.dmesh.mesh.ncells * self.nrt if self.output == 1 else self.ndofs

    def equilibrate_host(self, flux_dg, rhs_dg, flux_hdiv=None):
        """Host numpy arrays in/out; flux_hdiv [nrhs, ndofs] is accumulated (+=)."""
        m = self.dmesh.mesh
        g = np.ascontiguousarray(flux_dg, dtype=np.float64).reshape(self.nrhs, -1)
        f = np.ascontiguousarray(rhs_dg, dtype=np.float64).reshape(self.nrhs, -1)
        if g.shape[1] != m.ncells * self.nd * 2 or f.shape[1] != m.ncells * self.nd:
            raise RuntimeError("Equilibration: Input sizes does not match")
        if flux_hdiv is None:
            flux_hdiv = np.zeros((self.nrhs, self._nout()))
        assert flux_hdiv.dtype == np.float64 and flux_hdiv.flags.c_contiguous
        assert flux_hdiv.size == self.nrhs * self._nout()
        _check(lib().eqlb_ev_equilibrate(self._h, _hp(g), _hp(f), _hp(flux_hdiv),
                                         C.c_int32(MEM_HOST), None))
        return flux_hdiv

    def equilibrate_device(self, flux_dg_ptr: int, rhs_dg_ptr: int, flux_hdiv_ptr: int,
                           stream: int = 0):
        _check(lib().eqlb_ev_equilibrate(self._h, C.c_void_p(flux_dg_ptr), C.c_void_p(rhs_dg_ptr),
                                         C.c_void_p(flux_hdiv_ptr), C.c_int32(MEM_DEVICE),
                                         C.c_void_p(stream)))

    def check_status(self, stream: int = 0):
        _check(lib().eqlb_ev_check_status(self._h, C.c_void_p(stream)))

    def last_kernel_ms(self, which=0):
        return float(lib().eqlb_ev_last_kernel_ms(self._h, C.c_int32(which)))

    def close(self):
        if self._h:
            lib().eqlb_ev_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def reconstruct_fluxes_minimisation(flux_hdiv, flux_dg, rhs_dg, boundary_data):
    """Stand-in for `reconstruct_fluxes_minimisation(a, l_pen, l, flux_hdiv, boundary_data)`
    (wrappers.cpp:85-95): the forms a, l_pen, l of FluxEqlbEV.py:113-134 are fixed, their data
    (projected flux, projected RHS) is passed as flat arrays; `boundary_data` is a configured
    ConstrainedMinEquilibrator."""
    return boundary_data.equilibrate_host(flux_dg, rhs_dg, flux_hdiv)


def project_dg(dmesh: DeviceMesh, degree: int, qpoints, qweights, qvalues, bs: int = 1):
    """eqlb_project_dg on host arrays: qvalues [nrhs, ncells, nq, bs] -> DOFs [nrhs, ncells*nd*bs]."""
    m = dmesh.mesh
    qp = np.ascontiguousarray(qpoints, dtype=np.float64)
    qw = np.ascontiguousarray(qweights, dtype=np.float64)
    nq = qw.size
    qv = np.ascontiguousarray(qvalues, dtype=np.float64)
    if qv.size % (m.ncells * nq * bs) != 0:
        raise RuntimeError("Local solver: Input sizes does not match")
    nrhs = qv.size // (m.ncells * nq * bs)
    nd = (degree + 1) * (degree + 2) // 2
    out = np.zeros((nrhs, m.ncells * nd * bs))
    _check(lib().eqlb_project_dg(dmesh._h, C.c_int32(degree), C.c_int32(bs), C.c_int32(nrhs),
                                 C.c_int32(nq), _hp(qp), _hp(qw), _hp(qv), _hp(out),
                                 C.c_int32(MEM_HOST), None))
    return out


def _degree_dg(k: int, degree_dg):
    """Degree of the projected data of an estimator call (None: k-1, the entry points without _dg)."""
    if k < 1 or k > 4:
        raise RuntimeError(f"Equilibration: flux degree k = {k} outside 1 ... 4")
    if degree_dg is None:
        return k - 1
    if degree_dg < 0 or degree_dg > k - 1:
        raise RuntimeError("Equilibration: Wrong polynomial degree of the projected RHS")
    return int(degree_dg)


def estimate(dmesh: DeviceMesh, k: int, flux_hdiv, flux_dg, rhs_dg, conforming_flux=False, degree_dg=None, coeff=None,
             cell_D=None):
    """eqlb_se_estimate (eqlb_ev_estimate with conforming_flux=True: the flux is an EV result in
    the broken layout) on host arrays [nrhs, ...]: returns (cell_div2 [nrhs, ncells],
    cell_sig2 [nrhs, ncells], facet_jump [nrhs, nfacets]).  degree_dg: flux_dg / rhs_dg are DG_{degree_dg}
    data, 0 <= degree_dg <= k-1 (eqlb_se_estimate_dg / eqlb_ev_estimate_dg); None: DG_{k-1}.
    With coeff [ncells] and / or cell_D [ncells, 3] = (d00, d01, d11) (eqlb_se_estimate_weighted /
    eqlb_ev_estimate_weighted): cell_sig2 in the energy norm of -div(coeff D grad u), the integral of e^T W e with
    W = adj(D) / (coeff det D); cell_div2 and facet_jump are bit for bit those of the call without them
    (eqlb.check_eqlb_conditions.weighted_flux_norm is the statement).  The data oscillation takes the weight
    lsolver.primal.diffusion_oscillation_weight(cell_D, coeff).  Without the new keywords the call is the one it was."""
    m = dmesh.mesh
    deg = _degree_dg(k, degree_dg)
    nrt, nd = k * (k + 2), (deg + 1) * (deg + 2) // 2
    x = np.ascontiguousarray(flux_hdiv, dtype=np.float64).reshape(-1, m.ncells * nrt)
    nrhs = x.shape[0]
    g = np.ascontiguousarray(flux_dg, dtype=np.float64).reshape(nrhs, -1)
    f = np.ascontiguousarray(rhs_dg, dtype=np.float64).reshape(nrhs, -1)
    if g.shape[1] != m.ncells * nd * 2 or f.shape[1] != m.ncells * nd:
        raise RuntimeError("Equilibration: Input sizes does not match")
    div2 = np.zeros((nrhs, m.ncells))
    sig2 = np.zeros((nrhs, m.ncells))
    jump = np.zeros((nrhs, m.nfacets))
    if coeff is not None or cell_D is not None:
        kc = _cell_array(coeff, m.ncells)
        kd = None if cell_D is None else np.ascontiguousarray(cell_D, dtype=np.float64).ravel()
        if kd is not None and kd.size != 3 * m.ncells:
            raise RuntimeError("Equilibration: Input sizes does not match")
        estimate_weighted_raw(dmesh, k, deg, nrhs, _hp(x), _hp(g), _hp(f), None if kc is None else _hp(kc),
                              None if kd is None else _hp(kd), _hp(div2), _hp(sig2), _hp(jump), conforming_flux, MEM_HOST)
        return div2, sig2, jump
    estimate_raw(dmesh, k, nrhs, _hp(x), _hp(g), _hp(f), _hp(div2), _hp(sig2), _hp(jump), conforming_flux,
                 degree_dg, MEM_HOST)
    return div2, sig2, jump


def _vp(p):
    return p if p is None or isinstance(p, C.c_void_p) else C.c_void_p(p)


def estimate_raw(dmesh: DeviceMesh, k: int, nrhs: int, flux_hdiv, flux_dg, rhs_dg, cell_div2, cell_sig2, facet_jump,
                 conforming_flux=False, degree_dg=None, memspace=MEM_DEVICE, stream=0):
    """eqlb_se_estimate[_dg] / eqlb_ev_estimate[_dg] on raw pointers (ints or None for an output that is not
    wanted) in `memspace`, ordered on `stream`; device arrays stay where they are."""
    ptrs = [_vp(p) for p in (flux_hdiv, flux_dg, rhs_dg, cell_div2, cell_sig2, facet_jump)]
    tail = (C.c_int32(memspace), C.c_void_p(stream))
    if degree_dg is None:
        fn = lib().eqlb_ev_estimate if conforming_flux else lib().eqlb_se_estimate
        _check(fn(dmesh._h, C.c_int32(k), C.c_int32(nrhs), *ptrs, *tail))
    else:
        fn = lib().eqlb_ev_estimate_dg if conforming_flux else lib().eqlb_se_estimate_dg
        _check(fn(dmesh._h, C.c_int32(k), C.c_int32(degree_dg), C.c_int32(nrhs), *ptrs, *tail))


def estimate_weighted_raw(dmesh: DeviceMesh, k: int, degree_dg: int, nrhs: int, flux_hdiv, flux_dg, rhs_dg, cell_coeff,
                          cell_D, cell_div2, cell_sig2, facet_jump, conforming_flux=False, memspace=MEM_DEVICE,
                          stream=0):
    """eqlb_se_estimate_weighted / eqlb_ev_estimate_weighted on raw pointers (ints, or None for a coefficient that is
    not given / an output that is not wanted) in `memspace`, ordered on `stream`; degree_dg is explicit."""
    fn = lib().eqlb_ev_estimate_weighted if conforming_flux else lib().eqlb_se_estimate_weighted
    _check(fn(dmesh._h, C.c_int32(k), C.c_int32(degree_dg), C.c_int32(nrhs), _vp(flux_hdiv), _vp(flux_dg), _vp(rhs_dg),
              _vp(cell_coeff), _vp(cell_D), _vp(cell_div2), _vp(cell_sig2), _vp(facet_jump), C.c_int32(memspace),
              C.c_void_p(stream)))


def _cell_array(a, ncells):
    """A cell-wise coefficient as a contiguous float64 array [ncells], or None."""
    if a is None:
        return None
    v = np.ascontiguousarray(a, dtype=np.float64).ravel()
    if v.size != ncells:
        raise RuntimeError("Equilibration: Input sizes does not match")
    return v


def estimate_stress(dmesh: DeviceMesh, k: int, flux_hdiv, korn=None, pi_1: float = 1.0, cell_pi1=None,
                    mu: float = 1.0, cell_mu=None):
    """eqlb_se_estimate_stress on host arrays: flux_hdiv [2, ncells*k(k+2)] (rows of the equilibrated
    stress), korn [ncells] cell-wise Korn constants or None.  Returns (cell_energy [ncells],
    cell_wsym [ncells], node_asym [nnodes]).
    With cell_pi1 [ncells], mu or cell_mu [ncells] (eqlb_se_estimate_stress_mu): the terms for
    sigma = mu_T (2 eps(u) + pi_T div(u) I) - energy and wsym are formed with pi_T and divided by mu_T > 0, node_asym is
    unchanged.  The oscillation term takes the same weight through its own argument: oscillation(..., korn=korn /
    np.sqrt(cell_mu)).  A DG_0 coefficient crosses a refinement through Refinement.prolong_dg(0, ...).  Without the
    new keywords the call is the one it was."""
    m = dmesh.mesh
    if cell_pi1 is not None or cell_mu is not None or mu != 1.0:
        x = np.ascontiguousarray(flux_hdiv, dtype=np.float64)
        kc, kp, km = _cell_array(korn, m.ncells), _cell_array(cell_pi1, m.ncells), _cell_array(cell_mu, m.ncells)
        if x.size != 2 * m.ncells * k * (k + 2):
            raise RuntimeError("Equilibration: Input sizes does not match")
        energy, wsym, asym = np.zeros(m.ncells), np.zeros(m.ncells), np.zeros(m.nnodes)
        estimate_stress_mu_raw(dmesh, k, _hp(x), None if kc is None else _hp(kc), pi_1, None if kp is None else _hp(kp),
                               mu, None if km is None else _hp(km), _hp(energy), _hp(wsym), _hp(asym), MEM_HOST)
        return energy, wsym, asym
    x = np.ascontiguousarray(flux_hdiv, dtype=np.float64)
    if x.size != 2 * m.ncells * k * (k + 2):
        raise RuntimeError("Equilibration: Input sizes does not match")
    kc = None if korn is None else np.ascontiguousarray(korn, dtype=np.float64)
    if kc is not None and kc.size != m.ncells:
        raise RuntimeError("Equilibration: Input sizes does not match")
    energy, wsym, asym = np.zeros(m.ncells), np.zeros(m.ncells), np.zeros(m.nnodes)
    _check(lib().eqlb_se_estimate_stress(dmesh._h, C.c_int32(k), _hp(x), _hp(kc) if kc is not None else None,
                                         C.c_double(pi_1), _hp(energy), _hp(wsym), _hp(asym),
                                         C.c_int32(MEM_HOST), None))
    return energy, wsym, asym


def estimate_stress_mu_raw(dmesh: DeviceMesh, k: int, flux_hdiv, korn, pi_1: float, cell_pi1, mu: float, cell_mu,
                           cell_energy, cell_wsym, node_asym, memspace=MEM_DEVICE, stream=0):
    """eqlb_se_estimate_stress_mu on raw pointers (ints, or None for an array that is not given / an output that is not
    wanted) in `memspace`, ordered on `stream`."""
    _check(lib().eqlb_se_estimate_stress_mu(dmesh._h, C.c_int32(k), _vp(flux_hdiv), _vp(korn), C.c_double(pi_1),
                                            _vp(cell_pi1), C.c_double(mu), _vp(cell_mu), _vp(cell_energy),
                                            _vp(cell_wsym), _vp(node_asym), C.c_int32(memspace), C.c_void_p(stream)))


def oscillation(dmesh: DeviceMesh, k: int, flux, flux_dg, qpoints, qweights, fvalues, korn=None, degree_dg=None):
    """eqlb_oscillation on host arrays: flux [nrhs, ncells*k(k+2)], flux_dg [nrhs, ncells*nd*2] or None
    (conforming flux in the broken layout), fvalues [nrhs, ncells, nq].  Returns [nrhs, ncells].
    degree_dg: flux_dg is DG_{degree_dg} data (eqlb_oscillation_dg); None: DG_{k-1}."""
    m = dmesh.mesh
    deg = _degree_dg(k, degree_dg)
    x = np.ascontiguousarray(flux, dtype=np.float64).reshape(-1, m.ncells * k * (k + 2))
    nrhs = x.shape[0]
    g = None if flux_dg is None else np.ascontiguousarray(flux_dg, dtype=np.float64).reshape(nrhs, -1)
    qp = np.ascontiguousarray(qpoints, dtype=np.float64)
    qw = np.ascontiguousarray(qweights, dtype=np.float64)
    nq = qw.size
    fv = np.ascontiguousarray(fvalues, dtype=np.float64)
    if fv.size != nrhs * m.ncells * nq or (g is not None and g.shape[1] != m.ncells * (deg + 1) * (deg + 2)):
        raise RuntimeError("Equilibration: Input sizes does not match")
    kc = None if korn is None else np.ascontiguousarray(korn, dtype=np.float64)
    out = np.zeros((nrhs, m.ncells))
    oscillation_raw(dmesh, k, nrhs, _hp(x), _hp(g) if g is not None else None, qp, qw, _hp(fv),
                    _hp(kc) if kc is not None else None, _hp(out), degree_dg, MEM_HOST)
    return out


def oscillation_raw(dmesh: DeviceMesh, k: int, nrhs: int, flux, flux_dg, qpoints, qweights, fvalues, korn, out,
                    degree_dg=None, memspace=MEM_DEVICE, stream=0):
    """eqlb_oscillation[_dg] on raw pointers in `memspace`, ordered on `stream`; the rule (qpoints [nq, 2],
    qweights [nq]) is given as host arrays in either case."""
    qp = np.ascontiguousarray(qpoints, dtype=np.float64)
    qw = np.ascontiguousarray(qweights, dtype=np.float64)
    head = (dmesh._h, C.c_int32(k)) + (() if degree_dg is None else (C.c_int32(degree_dg),))
    fn = lib().eqlb_oscillation if degree_dg is None else lib().eqlb_oscillation_dg
    _check(fn(*head, C.c_int32(nrhs), _vp(flux), _vp(flux_dg), C.c_int32(qw.size), _hp(qp), _hp(qw), _vp(fvalues),
              _vp(korn), _vp(out), C.c_int32(memspace), C.c_void_p(stream)))


def boundary_residual(dmesh: DeviceMesh, k: int, flux, flux_dg, facets, boundary_values=None, degree_dg=None):
    """eqlb_boundary_residual on host arrays: per listed flux-BC facet the largest deviation of the facet DOFs of
    flux + flux_dg from the boundary DOFs (check_eqlb_conditions.boundary_flux_residual per facet).
    flux [nrhs, ncells*k(k+2)], flux_dg [nrhs, ncells*nd*2] in DG_{degree_dg} (None: k-1) or None (conforming
    flux in the broken layout), boundary_values [nrhs, ncells*k(k+2)] or None (homogeneous condition).
    Returns [nrhs, len(facets)]."""
    m = dmesh.mesh
    deg = _degree_dg(k, degree_dg)
    x = np.ascontiguousarray(flux, dtype=np.float64).reshape(-1, m.ncells * k * (k + 2))
    nrhs = x.shape[0]
    g = None if flux_dg is None else np.ascontiguousarray(flux_dg, dtype=np.float64).reshape(nrhs, -1)
    bv = None if boundary_values is None else np.ascontiguousarray(boundary_values, dtype=np.float64)
    if (g is not None and g.shape[1] != m.ncells * (deg + 1) * (deg + 2)) or (bv is not None and bv.size != x.size):
        raise RuntimeError("Equilibration: Input sizes does not match")
    fl = np.ascontiguousarray(facets, dtype=np.int32).reshape(-1)
    if fl.size and (fl.min() < 0 or fl.max() >= m.nfacets):
        raise RuntimeError("Equilibration: boundary facet outside the mesh")
    out = np.zeros((nrhs, fl.size))
    boundary_residual_raw(dmesh, k, deg, nrhs, _hp(x), _hp(g) if g is not None else None, fl.size, _hp(fl),
                          _hp(bv) if bv is not None else None, _hp(out), MEM_HOST)
    return out


def boundary_residual_raw(dmesh: DeviceMesh, k: int, degree_dg: int, nrhs: int, flux, flux_dg, nfacets_bc: int,
                          facets, boundary_values, out, memspace=MEM_DEVICE, stream=0):
    """eqlb_boundary_residual on raw pointers in `memspace` (facets: int32), ordered on `stream`."""
    _check(lib().eqlb_boundary_residual(dmesh._h, C.c_int32(k), C.c_int32(degree_dg), C.c_int32(nrhs), _vp(flux),
                                        _vp(flux_dg), C.c_int32(nfacets_bc), _vp(facets), _vp(boundary_values),
                                        _vp(out), C.c_int32(memspace), C.c_void_p(stream)))


def facet_points(dmesh: DeviceMesh, facets, s):
    """eqlb_facet_points on host arrays: physical points [nlist, nq, 2] of the facet parameters s on the listed
    boundary facets, seen from the facet's cell (eqlb.bcs._facet_points)."""
    fl = np.ascontiguousarray(facets, dtype=np.int32).ravel()
    ss, _ = _rule(s)
    out = np.zeros((fl.size, ss.size, 2))
    facet_points_raw(dmesh, fl.size, _hp(fl), ss, _hp(out), MEM_HOST)
    return out


def facet_points_raw(dmesh: DeviceMesh, nlist: int, facets, s, xq, memspace=MEM_DEVICE, stream=0):
    """eqlb_facet_points on raw pointers in `memspace` (facets int32, xq [nlist, nq, 2]); s is a host array."""
    ss, _ = _rule(s)
    _check(lib().eqlb_facet_points(dmesh._h, C.c_int32(nlist), _vp(facets), C.c_int32(ss.size), _hp(ss), _vp(xq),
                                   C.c_int32(memspace), C.c_void_p(stream)))


def flux_bc_dofs(dmesh: DeviceMesh, k: int, facets, s, w, values, vector=False):
    """eqlb_flux_bc_dofs on host arrays: facet DOFs [nlist, k] of the hierarchic RT_k from the point values
    [nlist, nq] of the normal flux, or [nlist, nq, 2] of a vector field with vector=True."""
    fl = np.ascontiguousarray(facets, dtype=np.int32).ravel()
    ss, ww = _rule(s, w)
    v = np.ascontiguousarray(values, dtype=np.float64)
    if v.size != fl.size * ss.size * (2 if vector else 1):
        raise RuntimeError("Equilibration: Input sizes does not match")
    out = np.zeros((fl.size, max(k, 0)))
    flux_bc_dofs_raw(dmesh, k, fl.size, _hp(fl), ss, ww, _hp(v), vector, _hp(out), MEM_HOST)
    return out


def flux_bc_dofs_raw(dmesh: DeviceMesh, k: int, nlist: int, facets, s, w, values, vector, dofs, memspace=MEM_DEVICE,
                     stream=0):
    """eqlb_flux_bc_dofs on raw pointers in `memspace`, ordered on `stream`; s, w are host arrays."""
    ss, ww = _rule(s, w)
    _check(lib().eqlb_flux_bc_dofs(dmesh._h, C.c_int32(k), C.c_int32(nlist), _vp(facets), C.c_int32(ss.size), _hp(ss),
                                   _hp(ww) if ww is not None else None, _vp(values), C.c_int32(1 if vector else 0),
                                   _vp(dofs), C.c_int32(memspace), C.c_void_p(stream)))


def indicator_total(terms, pair_last_two=False):
    """eqlb_indicator_total on host arrays: terms [nterms, ncells] squared cell-wise estimator terms (1 ... 8 of
    them).  Returns (cell_eta2 [ncells], totals [nterms + 1]): the sum of the terms per cell - with pair_last_two
    the last two enter as (sqrt a + sqrt b)^2 - and the sums over the cells of every term, then of cell_eta2
    (eqlb.marking.indicator_total is the numpy statement)."""
    t = [np.ascontiguousarray(v, dtype=np.float64).ravel() for v in terms]
    if not t or any(v.size != t[0].size for v in t):
        raise RuntimeError("Equilibration: Input sizes does not match")
    ncells = t[0].size
    eta2, totals = np.zeros(ncells), np.zeros(len(t) + 1)
    indicator_total_raw(ncells, [v.ctypes.data for v in t], pair_last_two, _hp(eta2), _hp(totals), MEM_HOST)
    return eta2, totals


def indicator_total_raw(ncells: int, terms, pair_last_two, cell_eta2, totals, memspace=MEM_DEVICE, stream=0):
    """eqlb_indicator_total on raw pointers (ints; None for an output that is not wanted) in `memspace`, ordered on
    `stream`: terms is a sequence of pointers to [ncells] arrays, totals [len(terms) + 1] lies in `memspace` too."""
    ptrs = (C.c_void_p * max(len(terms), 1))(*[p.value if isinstance(p, C.c_void_p) else p for p in terms])
    _check(lib().eqlb_indicator_total(C.c_int64(ncells), C.c_int32(len(terms)), ptrs,
                                      C.c_int32(1 if pair_last_two else 0), _vp(cell_eta2), _vp(totals),
                                      C.c_int32(memspace), C.c_void_p(stream)))


def mark_doerfler(cell_eta2, theta: float):
    """eqlb_mark_doerfler on a host array of non-negative indicators [ncells].  Returns (marked, eta2_total): the
    sorted int32 ids of the shortest list of cells, largest indicators first and equal ones in ascending id, whose
    sum exceeds theta * eta2_total (every cell if theta is 1 within 1e-8), and the sum of the indicators.  The
    list goes to the refiner as it is: DeviceMesh.refine(marked) refines on the device (from device memory:
    mark_doerfler_raw, then DeviceMesh.refine_raw on the same two pointers); a DOLFINx caller who refines on the host
    passes it to mesh.compute_incident_entities(mesh, marked, 2, 1) (eqlb.doerfler_marking is the numpy statement)."""
    eta = np.ascontiguousarray(cell_eta2, dtype=np.float64).ravel()
    marked = np.empty(max(eta.size, 1), dtype=np.int32)
    nmarked, total = C.c_int64(0), C.c_double(0.0)
    mark_doerfler_raw(eta.size, _hp(eta), theta, _hp(marked), C.addressof(nmarked), C.addressof(total), MEM_HOST)
    return marked[:nmarked.value].copy(), float(total.value)


def mark_doerfler_raw(ncells: int, cell_eta2, theta: float, marked, nmarked, eta2_total, memspace=MEM_DEVICE,
                      stream=0):
    """eqlb_mark_doerfler on raw pointers (ints; eta2_total may be None) in `memspace`, ordered on `stream`:
    marked [ncells] int32, nmarked [1] int64 and eta2_total [1] double lie in `memspace` too.  Device memory: nothing
    waits for the device; nmarked = -1 reports a negative or NaN indicator."""
    _check(lib().eqlb_mark_doerfler(C.c_int64(ncells), _vp(cell_eta2), C.c_double(theta), _vp(marked), _vp(nmarked),
                                    _vp(eta2_total), C.c_int32(memspace), C.c_void_p(stream)))


def _primal_sizes(p: int, degree_dg: int):
    if p < 1 or p > 4 or degree_dg < 0 or degree_dg > 3:
        raise RuntimeError(f"Local solver: degrees p = {p}, degree_dg = {degree_dg} outside 1 ... 4, 0 ... 3")
    return (p + 1) * (p + 2) // 2, (degree_dg + 1) * (degree_dg + 2) // 2


def _primal_op(op, nd, ndp):
    if op is None:
        return None
    t = np.ascontiguousarray(op, dtype=np.float64)
    if t.size != 2 * nd * ndp:
        raise RuntimeError("Local solver: Input sizes does not match")
    return t


def get_primal_table(p: int, degree_dg: int):
    """The built-in table PG<p,d> [2, nd_d, nd_p] of primal_flux_dg (eqlb_get_primal_table): DG_d DOFs of the
    reference gradient of the P_p basis functions (tools/gen_tables.py: primal_table_exact)."""
    ndp, nd = (p + 1) * (p + 2) // 2, (degree_dg + 1) * (degree_dg + 2) // 2
    out = np.zeros(max(2 * nd * ndp, 1))
    n = lib().eqlb_get_primal_table(C.c_int32(p), C.c_int32(degree_dg), _hp(out), C.c_int32(out.size))
    if n < 0:
        raise RuntimeError(lib().eqlb_last_error().decode())
    return out[:n].reshape(2, nd, ndp)


def get_prolong_table(q: int):
    """The built-in table PT<q> [(2q+1)(q+1), nd_q] of the prolongation (eqlb_get_prolong_table), 1 <= q <= 4."""
    nrow, nd = (2 * max(q, 0) + 1) * (max(q, 0) + 1), (max(q, 0) + 1) * (max(q, 0) + 2) // 2
    out = np.zeros((nrow, nd))
    n = lib().eqlb_get_prolong_table(C.c_int32(q), _hp(out), C.c_int32(out.size))
    if n < 0:
        _check(n)
    return out


def get_flux_bc_prolong_table(k: int):
    """The built-in table FB<k> [6, k, k] of the flux-BC prolongation (eqlb_get_flux_bc_prolong_table), 1 <= k <= 4."""
    kk = max(int(k), 1)
    out = np.zeros((6, kk, kk))
    n = lib().eqlb_get_flux_bc_prolong_table(C.c_int32(k), _hp(out), C.c_int32(out.size))
    if n < 0:
        _check(n)
    return out


def primal_flux_dg(dmesh: DeviceMesh, p: int, degree_dg: int, cell_dofs, u, coeff=None, op=None, cell_D=None):
    """eqlb_primal_flux_dg on host arrays: the DG_{degree_dg}^2 DOFs of -coeff grad(u_h) for u_h in P_p given by
    its cell dofmap cell_dofs [ncells, nd_p] and solution vectors u [nrhs, ndofs] (or [ndofs]); coeff [ncells]
    or None (1); op [2, nd_d, nd_p] replaces the built-in table.  Returns [nrhs, ncells*nd_d*2].
    With cell_D [ncells, 3] = (d00, d01, d11) (eqlb_primal_flux_dg_tensor): the flux -coeff D grad(u_h) of
    PrimalPoisson.set_diffusion; lsolver.primal.flux_dg_tensor is its statement.  Without it the call is the one it
    was."""
    m = dmesh.mesh
    ndp, nd = _primal_sizes(p, degree_dg)
    cd = np.ascontiguousarray(cell_dofs, dtype=np.int32)
    uu = np.ascontiguousarray(u, dtype=np.float64)
    uu = uu.reshape(1, -1) if uu.ndim < 2 else uu.reshape(uu.shape[0], -1)
    kc = None if coeff is None else np.ascontiguousarray(coeff, dtype=np.float64)
    if cd.size != m.ncells * ndp or uu.size == 0 or (kc is not None and kc.size != m.ncells):
        raise RuntimeError("Local solver: Input sizes does not match")
    t = _primal_op(op, nd, ndp)
    out = np.zeros((uu.shape[0], m.ncells * nd * 2))
    if cell_D is not None:
        kd = np.ascontiguousarray(cell_D, dtype=np.float64).ravel()
        if kd.size != 3 * m.ncells:
            raise RuntimeError("Local solver: Input sizes does not match")
        primal_flux_dg_tensor_raw(dmesh, p, degree_dg, uu.shape[0], _hp(cd), uu.shape[1], _hp(uu),
                                  _hp(kc) if kc is not None else None, _hp(kd), _hp(out), t, MEM_HOST)
        return out
    primal_flux_dg_raw(dmesh, p, degree_dg, uu.shape[0], _hp(cd), uu.shape[1], _hp(uu),
                       _hp(kc) if kc is not None else None, _hp(out), t, MEM_HOST)
    return out


def primal_flux_dg_tensor_raw(dmesh: DeviceMesh, p: int, degree_dg: int, nrhs: int, cell_dofs, ndofs: int, u, coeff,
                              cell_D, flux_dg, op=None, memspace=MEM_DEVICE, stream=0):
    """eqlb_primal_flux_dg_tensor on raw pointers (ints; coeff may be None) in `memspace`, ordered on `stream`: the
    arrays of primal_flux_dg_raw and cell_D [ncells, 3].  Device memory: one kernel, nothing waits for the device."""
    t = None if op is None else np.ascontiguousarray(op, dtype=np.float64)
    _check(lib().eqlb_primal_flux_dg_tensor(dmesh._h, C.c_int32(p), C.c_int32(degree_dg), C.c_int32(nrhs),
                                            _vp(cell_dofs), C.c_int64(ndofs), _vp(u), _vp(coeff), _vp(cell_D),
                                            _hp(t) if t is not None else None, _vp(flux_dg), C.c_int32(memspace),
                                            C.c_void_p(stream)))


def primal_flux_dg_raw(dmesh: DeviceMesh, p: int, degree_dg: int, nrhs: int, cell_dofs, ndofs: int, u, coeff,
                       flux_dg, op=None, memspace=MEM_DEVICE, stream=0):
    """eqlb_primal_flux_dg on raw pointers (ints; coeff may be None) in `memspace`, ordered on `stream`: cell_dofs
    int32 [ncells, nd_p], u [nrhs, ndofs], flux_dg [nrhs, ncells*nd_d*2].  op is a host array or None.  Device
    memory: one kernel, nothing waits for the device."""
    t = None if op is None else np.ascontiguousarray(op, dtype=np.float64)
    _check(lib().eqlb_primal_flux_dg(dmesh._h, C.c_int32(p), C.c_int32(degree_dg), C.c_int32(nrhs), _vp(cell_dofs),
                                     C.c_int64(ndofs), _vp(u), _vp(coeff), _hp(t) if t is not None else None,
                                     _vp(flux_dg), C.c_int32(memspace), C.c_void_p(stream)))


def primal_stress_dg(dmesh: DeviceMesh, p: int, degree_dg: int, cell_dofs, u, pi_1: float = 1.0, cell_pi1=None,
                     op=None, mu: float = 1.0, cell_mu=None):
    """eqlb_primal_stress_dg on host arrays: rows of -(2 eps(u_h) + pi_1 div(u_h) I) for the blocked displacement
    u [ndofs, 2] in P_p^2 (scalar dofmap cell_dofs), pi_1 per cell where cell_pi1 [ncells] is given.  Returns
    [2, ncells*nd_d*2].  With mu or cell_mu [ncells] (eqlb_primal_stress_dg_mu): rows of -mu_T (2 eps(u_h) + pi_1
    div(u_h) I), every value mu_T > 0 times the value formed without it, rounded once; a DG_0 cell_mu crosses a
    refinement through Refinement.prolong_dg(0, ...).  Without the new keywords the call is the one it was."""
    m = dmesh.mesh
    ndp, nd = _primal_sizes(p, degree_dg)
    cd = np.ascontiguousarray(cell_dofs, dtype=np.int32)
    uu = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
    kc = None if cell_pi1 is None else np.ascontiguousarray(cell_pi1, dtype=np.float64)
    if cd.size != m.ncells * ndp or uu.size == 0 or uu.size % 2 or (kc is not None and kc.size != m.ncells):
        raise RuntimeError("Local solver: Input sizes does not match")
    t = _primal_op(op, nd, ndp)
    out = np.zeros((2, m.ncells * nd * 2))
    if cell_mu is not None or mu != 1.0:
        km = None if cell_mu is None else np.ascontiguousarray(cell_mu, dtype=np.float64).ravel()
        if km is not None and km.size != m.ncells:
            raise RuntimeError("Local solver: Input sizes does not match")
        primal_stress_dg_mu_raw(dmesh, p, degree_dg, _hp(cd), uu.size // 2, _hp(uu), pi_1,
                                _hp(kc) if kc is not None else None, mu, _hp(km) if km is not None else None,
                                _hp(out), t, MEM_HOST)
        return out
    primal_stress_dg_raw(dmesh, p, degree_dg, _hp(cd), uu.size // 2, _hp(uu), pi_1,
                         _hp(kc) if kc is not None else None, _hp(out), t, MEM_HOST)
    return out


def primal_stress_dg_raw(dmesh: DeviceMesh, p: int, degree_dg: int, cell_dofs, ndofs: int, u, pi_1: float, cell_pi1,
                         flux_dg, op=None, memspace=MEM_DEVICE, stream=0):
    """eqlb_primal_stress_dg on raw pointers (ints; cell_pi1 may be None) in `memspace`, ordered on `stream`:
    u [ndofs, 2] blocked, flux_dg [2, ncells*nd_d*2]."""
    t = None if op is None else np.ascontiguousarray(op, dtype=np.float64)
    _check(lib().eqlb_primal_stress_dg(dmesh._h, C.c_int32(p), C.c_int32(degree_dg), _vp(cell_dofs),
                                       C.c_int64(ndofs), _vp(u), C.c_double(pi_1), _vp(cell_pi1),
                                       _hp(t) if t is not None else None, _vp(flux_dg), C.c_int32(memspace),
                                       C.c_void_p(stream)))


def primal_stress_dg_mu_raw(dmesh: DeviceMesh, p: int, degree_dg: int, cell_dofs, ndofs: int, u, pi_1: float, cell_pi1,
                            mu: float, cell_mu, flux_dg, op=None, memspace=MEM_DEVICE, stream=0):
    """eqlb_primal_stress_dg_mu on raw pointers (ints; cell_pi1 and cell_mu may be None) in `memspace`, ordered on
    `stream`: u [ndofs, 2] blocked, flux_dg [2, ncells*nd_d*2]."""
    t = None if op is None else np.ascontiguousarray(op, dtype=np.float64)
    _check(lib().eqlb_primal_stress_dg_mu(dmesh._h, C.c_int32(p), C.c_int32(degree_dg), _vp(cell_dofs),
                                          C.c_int64(ndofs), _vp(u), C.c_double(pi_1), _vp(cell_pi1), C.c_double(mu),
                                          _vp(cell_mu), _hp(t) if t is not None else None, _vp(flux_dg),
                                          C.c_int32(memspace), C.c_void_p(stream)))


def get_value_table(p: int, degree_dg: int):
    """The built-in table PV<p,d> [nd_d, nd_p] of primal_value_dg (eqlb_get_value_table): DG_d nodal values of the L2
    projection of the P_p basis functions onto P_d (lsolver.primal.value_table_exact)."""
    ndp, nd = (max(int(p), 0) + 1) * (max(int(p), 0) + 2) // 2, (max(int(degree_dg), 0) + 1) * (max(int(degree_dg), 0) + 2) // 2
    out = np.zeros((nd, ndp))
    n = lib().eqlb_get_value_table(C.c_int32(p), C.c_int32(degree_dg), _hp(out), C.c_int32(out.size))
    if n < 0:
        _check(n)
    return out


def primal_value_dg(dmesh: DeviceMesh, p: int, degree_dg: int, cell_dofs, u, coeff=None, op=None):
    """eqlb_primal_value_dg on host arrays: the DG_{degree_dg} DOFs of coeff Pi_d u_h for u_h in P_p given by its cell
    dofmap cell_dofs [ncells, nd_p] and vectors u [nrhs, ndofs] (or [ndofs]); coeff [ncells] or None (no
    multiplication); op [nd_d, nd_p] replaces the built-in table.  Returns [nrhs, ncells*nd_d]: with coeff = c_T the
    reaction part of the right-hand side an equilibrator needs, rhs = Pi_d f - primal_value_dg(u_h, c)."""
    m = dmesh.mesh
    ndp, nd = _primal_sizes(p, degree_dg)
    cd = np.ascontiguousarray(cell_dofs, dtype=np.int32)
    uu = np.ascontiguousarray(u, dtype=np.float64)
    uu = uu.reshape(1, -1) if uu.ndim < 2 else uu.reshape(uu.shape[0], -1)
    kc = None if coeff is None else np.ascontiguousarray(coeff, dtype=np.float64)
    if cd.size != m.ncells * ndp or uu.size == 0 or (kc is not None and kc.size != m.ncells):
        raise RuntimeError("Local solver: Input sizes does not match")
    t = None
    if op is not None:
        t = np.ascontiguousarray(op, dtype=np.float64)
        if t.size != nd * ndp:
            raise RuntimeError("Local solver: Input sizes does not match")
    out = np.zeros((uu.shape[0], m.ncells * nd))
    primal_value_dg_raw(dmesh, p, degree_dg, uu.shape[0], _hp(cd), uu.shape[1], _hp(uu),
                        _hp(kc) if kc is not None else None, _hp(out), t, MEM_HOST)
    return out


def primal_value_dg_raw(dmesh: DeviceMesh, p: int, degree_dg: int, nrhs: int, cell_dofs, ndofs: int, u, coeff,
                        value_dg, op=None, memspace=MEM_DEVICE, stream=0):
    """eqlb_primal_value_dg on raw pointers (ints; coeff may be None) in `memspace`, ordered on `stream`: cell_dofs
    int32 [ncells, nd_p], u [nrhs, ndofs], value_dg [nrhs, ncells*nd_d].  op is a host array or None.  Device memory:
    one kernel, nothing waits for the device."""
    t = None if op is None else np.ascontiguousarray(op, dtype=np.float64)
    _check(lib().eqlb_primal_value_dg(dmesh._h, C.c_int32(p), C.c_int32(degree_dg), C.c_int32(nrhs), _vp(cell_dofs),
                                      C.c_int64(ndofs), _vp(u), _vp(coeff), _hp(t) if t is not None else None,
                                      _vp(value_dg), C.c_int32(memspace), C.c_void_p(stream)))


def get_mass_table(p: int):
    """The built-in table Mass<p> [nd_p, nd_p] of the reaction term (eqlb_get_mass_table), 1 <= p <= 4."""
    nd = (max(int(p), 0) + 1) * (max(int(p), 0) + 2) // 2
    out = np.zeros((nd, nd))
    n = lib().eqlb_get_mass_table(C.c_int32(p), _hp(out), C.c_int32(out.size))
    if n < 0:
        _check(n)
    return out


def get_facet_mass_table(p: int):
    """The built-in table FacetMass<p> [p+1, p+1] of the Robin term (eqlb_get_facet_mass_table), 1 <= p <= 4."""
    n1 = max(int(p), 0) + 1
    out = np.zeros((n1, n1))
    n = lib().eqlb_get_facet_mass_table(C.c_int32(p), _hp(out), C.c_int32(out.size))
    if n < 0:
        _check(n)
    return out


def get_stiffness_table(p: int):
    """The built-in table Stiff<p> [3, nd_p, nd_p] of PrimalPoisson (eqlb_get_stiffness_table), 1 <= p <= 4."""
    nd = (max(int(p), 0) + 1) * (max(int(p), 0) + 2) // 2
    out = np.zeros((3, nd, nd))
    n = lib().eqlb_get_stiffness_table(C.c_int32(p), _hp(out), C.c_int32(out.size))
    if n < 0:
        _check(n)
    return out


def get_load_table(p: int, degree_dg: int):
    """The built-in table Load<p,d> [nd_p, nd_d] of PrimalPoisson.load (eqlb_get_load_table)."""
    ndp, nd = (max(int(p), 0) + 1) * (max(int(p), 0) + 2) // 2, (max(int(degree_dg), 0) + 1) * (max(int(degree_dg), 0) + 2) // 2
    out = np.zeros((ndp, nd))
    n = lib().eqlb_get_load_table(C.c_int32(p), C.c_int32(degree_dg), _hp(out), C.c_int32(out.size))
    if n < 0:
        _check(n)
    return out


def get_cross_table(p: int):
    """The built-in table Cross<p> [nd_p, nd_p] of PrimalElasticity (eqlb_get_cross_table), 1 <= p <= 4."""
    nd = (max(int(p), 0) + 1) * (max(int(p), 0) + 2) // 2
    out = np.zeros((nd, nd))
    n = lib().eqlb_get_cross_table(C.c_int32(p), _hp(out), C.c_int32(out.size))
    if n < 0:
        _check(n)
    return out


PRIMAL_INFO = ("iterations", "converged", "nb", "rnorm", "replacements", "breakdown", "tol", "facets_skipped")


def _primal_info(v):
    info = dict(zip(PRIMAL_INFO, [float(x) for x in v]))
    for key in ("iterations", "converged", "replacements", "breakdown", "facets_skipped"):
        info[key] = int(info[key])
    return info


def _columns(a, n):
    """[nrhs][n] as one contiguous array; the column count comes from the array"""
    v = np.ascontiguousarray(a, dtype=np.float64)
    if v.ndim != 2 or v.shape[0] < 1 or v.shape[1] != n:
        raise RuntimeError("Local solver: Input sizes does not match")
    return v


class _PrimalSolver:
    """What PrimalPoisson and PrimalElasticity share: the entries of the C ABI that differ by the symbol prefix and by
    the vector length _bs * ndofs only.  A subclass creates the handle `_h` and sets `dmesh`, `p`, `ndofs`."""

    _prefix = None   # "eqlb_primal_" / "eqlb_elasticity_"
    _bs = None       # components per DOF

    def _fn(self, name):
        return getattr(lib(), self._prefix + name)

    def _read_ndofs(self):
        n = C.c_int64(0)
        _check(self._fn("ndofs")(self._h, C.byref(n)))
        self.ndofs = int(n.value)

    def _vec(self, a):
        v = np.ascontiguousarray(a, dtype=np.float64).ravel()
        if v.size != self._bs * self.ndofs:
            raise RuntimeError("Local solver: Input sizes does not match")
        return v

    def load(self, degree_dg, rhs_dg, b_extra=None, stream=0):
        """b [bs ndofs] from the DG_d nodal values rhs_dg [bs][ncells * nd_d] of the bs components (1: Poisson,
        2: elasticity), + b_extra [bs ndofs] where given (elasticity: lsolver.traction_load)."""
        d = max(int(degree_dg), 0)
        f = np.ascontiguousarray(rhs_dg, dtype=np.float64).ravel()
        if 0 <= degree_dg <= 3 and f.size != self._bs * self.dmesh.counts()[1] * (d + 1) * (d + 2) // 2:
            raise RuntimeError("Local solver: Input sizes does not match")
        e = None if b_extra is None else self._vec(b_extra)
        b = np.zeros(self._bs * self.ndofs)
        self.load_raw(degree_dg, f.ctypes.data, None if e is None else e.ctypes.data, b.ctypes.data, MEM_HOST, stream)
        return b

    def load_raw(self, degree_dg, rhs_dg, b_extra, b, memspace=MEM_DEVICE, stream=0):
        _check(self._fn("load")(self._h, C.c_int32(degree_dg), _vp(rhs_dg), _vp(b_extra), _vp(b),
                                C.c_int32(memspace), C.c_void_p(stream)))

    def set_reaction(self, c=0.0, cell_c=None, stream=0):
        """The operator gains + c u (eqlb_primal_set_reaction / eqlb_elasticity_set_reaction): cell_c, a host array
        [ncells], where given, else the scalar c on every cell; c == 0 without an array switches the term off.  A
        repeated call replaces the coefficient; a negative, NaN or infinite one is refused and the handle stays as it
        was.  The diagonal is formed again; Multilevel.set_coarse(True) has to be called again afterwards."""
        kc = None
        if cell_c is not None:
            kc = np.ascontiguousarray(cell_c, dtype=np.float64).ravel()
            if kc.size != self.dmesh.counts()[1]:
                raise RuntimeError("Local solver: Input sizes does not match")
        self.set_reaction_raw(c, None if kc is None else kc.ctypes.data, MEM_HOST, stream)

    def set_reaction_raw(self, c=0.0, cell_c=None, memspace=MEM_DEVICE, stream=0):
        """cell_c: a raw pointer (int) to [ncells] in `memspace`, or None (the scalar c)."""
        _check(self._fn("set_reaction")(self._h, C.c_double(c), _vp(cell_c), C.c_int32(memspace), C.c_void_p(stream)))

    # ---- the facet term: the Robin term of PrimalPoisson, the spring term of PrimalElasticity.  A subclass names it in
    # _facet = (setter, stem, width): the entries set_<...>, <stem>_weights and <stem>_flux of the C ABI, the public
    # names <setter>, <stem>_list in messages, and the values per listed facet (alpha: 1, (k00, k01, k11): 3).  The
    # flux has _bs rows.  The public methods of the subclasses are thin calls of these.
    _facet = None

    def _facet_set(self, facets, scalar_row, values, stream):
        """The list from host arrays; values [nlist, width] or None: scalar_row [width] on every facet.  The accepted
        list is remembered for <stem>_list()."""
        width = self._facet[2]
        fl = np.ascontiguousarray(facets, dtype=np.int32).ravel()
        fv = None
        if values is not None:
            fv = np.ascontiguousarray(values, dtype=np.float64).ravel()
            if fv.size != width * fl.size:
                raise RuntimeError("Local solver: Input sizes does not match")
        self._facet_set_raw(fl.size, fl.ctypes.data if fl.size else None, scalar_row[0],
                            fv.ctypes.data if fv is not None and fv.size else None, MEM_HOST, stream)
        rows = np.tile(np.asarray(scalar_row, dtype=np.float64), (fl.size, 1)) if fv is None else fv.copy()
        self._facet_known = (fl.copy(), rows.reshape(self._facet_shape(fl.size)))

    def _facet_shape(self, n):
        return (n,) if self._facet[2] == 1 else (n, self._facet[2])

    def _facet_list(self):
        """(facets, values) as the last accepted host setter took them; empty without the term.  A handle whose
        non-empty list came through the raw setter is refused: the host does not know that list."""
        setter, stem, _ = self._facet
        known = getattr(self, "_facet_known", None)
        if known is None or known[0].size != self._facet_count():
            if self._facet_count() != 0:
                raise RuntimeError(f"{stem}_list: the handle's list was not given through {setter} (host arrays)")
            return np.zeros(0, dtype=np.int32), np.zeros(self._facet_shape(0))
        return known

    def _facet_set_raw(self, nlist, facets, scalar, values, memspace, stream):
        _check(self._fn(self._facet[0])(self._h, C.c_int32(nlist), _vp(facets), C.c_double(scalar), _vp(values),
                                        C.c_int32(memspace), C.c_void_p(stream)))
        self._facet_known = None   # (a refused call has left the handle, and so the remembered list, as it was)

    def _facet_count(self):
        return self._facet_weights_raw(None, 0, MEM_HOST, 0)

    def _facet_weights(self, stream):
        w = np.zeros(self._facet_shape(self._facet_count()))
        if w.size:
            self._facet_weights_raw(w.ctypes.data, w.shape[0], MEM_HOST, stream)
        return w

    def _facet_weights_raw(self, w, capacity, memspace, stream):
        n = C.c_int32(0)
        _check(self._fn(self._facet[1] + "_weights")(self._h, C.byref(n), _vp(w), C.c_int32(capacity),
                                                     C.c_int32(memspace), C.c_void_p(stream)))
        return int(n.value)

    def _facet_flux(self, u, s, u_ext, stream):
        uu = self._vec(u)
        ss = np.ascontiguousarray(s, dtype=np.float64).ravel()
        shape = (self._facet_count(), ss.size) if self._bs == 1 else (self._bs, self._facet_count(), ss.size)
        ue = None
        if u_ext is not None:
            ue = np.ascontiguousarray(u_ext, dtype=np.float64).ravel()
            if ue.size != int(np.prod(shape)):
                raise RuntimeError("Local solver: Input sizes does not match")
        out = np.zeros(shape)
        self._facet_flux_raw(uu.ctypes.data, ss, None if ue is None else ue.ctypes.data, out.ctypes.data, MEM_HOST,
                             stream)
        return out

    def _facet_flux_raw(self, u, s, u_ext, out, memspace, stream):
        ss = np.ascontiguousarray(s, dtype=np.float64).ravel()
        _check(self._fn(self._facet[1] + "_flux")(self._h, _vp(u), C.c_int32(ss.size), _hp(ss), _vp(u_ext), _vp(out),
                                                  C.c_int32(memspace), C.c_void_p(stream)))

    def apply(self, u, masked=False, stream=0):
        """y = A u; masked: 0 on the fixed rows."""
        uu, y = self._vec(u), np.zeros(self._bs * self.ndofs)
        self.apply_raw(uu.ctypes.data, y.ctypes.data, masked, MEM_HOST, stream)
        return y

    def apply_raw(self, u, y, masked=False, memspace=MEM_DEVICE, stream=0):
        _check(self._fn("apply")(self._h, _vp(u), _vp(y), C.c_int32(1 if masked else 0), C.c_int32(memspace),
                                 C.c_void_p(stream)))

    def diagonal(self, stream=0):
        out = np.zeros(self._bs * self.ndofs)
        self.diagonal_raw(out.ctypes.data, MEM_HOST, stream)
        return out

    def diagonal_raw(self, out, memspace=MEM_DEVICE, stream=0):
        _check(self._fn("diagonal")(self._h, _vp(out), C.c_int32(memspace), C.c_void_p(stream)))

    def residual(self, b, u, norms=False, stream=0):
        """r = b - A u with 0 on the fixed rows; norms=True: (r, || r ||_2, nb)."""
        bb, uu, r = self._vec(b), self._vec(u), np.zeros(self._bs * self.ndofs)
        nv = np.zeros(2)
        self.residual_raw(bb.ctypes.data, uu.ctypes.data, r.ctypes.data, nv.ctypes.data if norms else None, MEM_HOST,
                          stream)
        return (r, float(nv[0]), float(nv[1])) if norms else r

    def residual_raw(self, b, u, r, norms=None, memspace=MEM_DEVICE, stream=0):
        _check(self._fn("residual")(self._h, _vp(b), _vp(u), _vp(r), _vp(norms), C.c_int32(memspace),
                                    C.c_void_p(stream)))

    def solve(self, b, u, rtol=1e-8, atol=0.0, maxit=10000, stream=0):
        """Jacobi-preconditioned CG from the start u (its fixed rows hold the Dirichlet values).  Returns (u, info):
        the solution and a dict with the keys of PRIMAL_INFO.  Not converged is a result, not an error."""
        bb = self._vec(b)
        uu = self._vec(u).copy()
        info = self.solve_raw(bb.ctypes.data, uu.ctypes.data, rtol, atol, maxit, MEM_HOST, stream)
        return uu, info

    def solve_raw(self, b, u, rtol=1e-8, atol=0.0, maxit=10000, memspace=MEM_DEVICE, stream=0):
        """eqlb_primal_solve / eqlb_elasticity_solve on raw pointers: u is overwritten by the solution; waits for the
        device; returns info."""
        v = (C.c_double * 8)()
        _check(self._fn("solve")(self._h, _vp(b), _vp(u), C.c_double(rtol), C.c_double(atol), C.c_int32(maxit), v,
                                 C.c_int32(memspace), C.c_void_p(stream)))
        return _primal_info(v)

    # ---- the operator as CSR (eqlb_primal_matrix_* / eqlb_elasticity_matrix_*; lsolver.primal: matrix, csr_apply) ----
    def matrix_pattern_raw(self, stream=0):
        """nnz: builds the pattern on `stream` at the first call (which waits for the count), then it is cached."""
        n = C.c_int64(0)
        _check(self._fn("matrix_pattern")(self._h, C.byref(n), C.c_void_p(stream)))
        return int(n.value)

    def matrix_export_raw(self, indptr, indices, memspace=MEM_DEVICE, stream=0):
        """indptr int64 [bs ndofs + 1] and indices int32 [nnz] behind raw pointers in `memspace`."""
        _check(self._fn("matrix_export")(self._h, _vp(indptr), _vp(indices), C.c_int32(memspace), C.c_void_p(stream)))

    def matrix_values_raw(self, eliminate, values, capacity, memspace=MEM_DEVICE, stream=0):
        """values float64 [nnz] behind a raw pointer in `memspace`, from what the handle holds now."""
        _check(self._fn("matrix_values")(self._h, C.c_int32(eliminate), _vp(values), C.c_int64(capacity),
                                         C.c_int32(memspace), C.c_void_p(stream)))

    def matrix_values(self, eliminate=False, device=False, stream=0):
        """values [nnz] of the matrix from the coefficients, the terms and the mask the handle has now: the refill after
        set_reaction, set_shear, set_diffusion or set_dirichlet, on the pattern as it stands.  eliminate: P A P + (I - P)
        on the mask.  device=True: a torch tensor on the device, written on `stream`."""
        flag = int(eliminate) if isinstance(eliminate, (bool, int, np.integer)) else -1
        nnz = self.matrix_pattern_raw(stream)
        if device:
            import torch
            v = torch.empty(nnz, dtype=torch.float64, device="cuda")
            self.matrix_values_raw(flag, v.data_ptr(), nnz, MEM_DEVICE, stream)
            return v
        v = np.zeros(nnz)
        self.matrix_values_raw(flag, v.ctypes.data, nnz, MEM_HOST, stream)
        return v

    def matrix(self, eliminate=False, device=False, stream=0):
        """(indptr int64 [n + 1], indices int32 [nnz], values float64 [nnz]), n = bs ndofs: the operator as CSR,
        scipy.sparse.csr_matrix((values, indices, indptr), shape=(n, n)); lsolver.primal states the rule, the arrays
        have its bits.  The pattern is built at the first call and kept in the handle (matrix_release frees it).
        device=True: torch tensors on the device, written on `stream`."""
        nnz = self.matrix_pattern_raw(stream)
        n = self._bs * self.ndofs
        if device:
            import torch
            ip = torch.empty(n + 1, dtype=torch.int64, device="cuda")
            ix = torch.empty(nnz, dtype=torch.int32, device="cuda")
            self.matrix_export_raw(ip.data_ptr(), ix.data_ptr(), MEM_DEVICE, stream)
        else:
            ip, ix = np.zeros(n + 1, dtype=np.int64), np.zeros(nnz, dtype=np.int32)
            self.matrix_export_raw(ip.ctypes.data, ix.ctypes.data, MEM_HOST, stream)
        return ip, ix, self.matrix_values(eliminate, device, stream)

    def matrix_release(self):
        """Frees the cached pattern; the next matrix() builds it again."""
        self._fn("matrix_release")(self._h)

    def close(self):
        if self._h:
            self._fn("destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def csr_apply_raw(n, indptr, indices, values, x, y, memspace=MEM_DEVICE, stream=0):
    """eqlb_csr_apply on raw pointers in `memspace`."""
    _check(lib().eqlb_csr_apply(C.c_int64(n), _vp(indptr), _vp(indices), _vp(values), _vp(x), _vp(y),
                                C.c_int32(memspace), C.c_void_p(stream)))


def csr_apply(indptr, indices, values, x, stream=0):
    """y = A x for a CSR matrix on the device (eqlb_csr_apply; lsolver.primal.csr_apply states the sum): host arrays, or
    torch tensors on the device (int64, int32, float64, float64), which are read on `stream`."""
    if not isinstance(x, np.ndarray) and hasattr(x, "data_ptr"):
        import torch
        y = torch.empty_like(x)
        csr_apply_raw(x.numel(), indptr.data_ptr(), indices.data_ptr(), values.data_ptr(), x.data_ptr(), y.data_ptr(),
                      MEM_DEVICE, stream)
        return y
    ip = np.ascontiguousarray(indptr, dtype=np.int64).ravel()
    ix = np.ascontiguousarray(indices, dtype=np.int32).ravel()
    v = np.ascontiguousarray(values, dtype=np.float64).ravel()
    xx = np.ascontiguousarray(x, dtype=np.float64).ravel()
    if ip.size != xx.size + 1 or ix.size != v.size or (ip.size and int(ip[-1]) != v.size):
        raise RuntimeError("csr_apply: Input sizes does not match")
    y = np.zeros(xx.size)
    csr_apply_raw(xx.size, ip.ctypes.data, ix.ctypes.data, v.ctypes.data, xx.ctypes.data, y.ctypes.data, MEM_HOST,
                  stream)
    return y


class PrimalPoisson(_PrimalSolver):
    """eqlb_primal_t: -div(coeff grad u) = f on the conforming P_p space of the handle (1 <= p <= 4), in the numbering
    of DeviceMesh.lagrange_dofmap: the operator matrix-free, the load vector, the residual and a Jacobi-preconditioned
    CG on the device (lsolver.primal.PoissonOperator is the numpy statement).  coeff: host array [ncells] or None (1).
    The methods take and return host arrays; the `_raw` variants take raw pointers (ints) in `memspace`, ordered on
    `stream`.  The entries of one handle share its work space: one stream, one call after the other."""

    _prefix, _bs = "eqlb_primal_", 1
    _facet = ("set_robin", "robin", 1)

    def __init__(self, dmesh: DeviceMesh, p: int, coeff=None, stream=0):
        self.dmesh = dmesh   # the handle reads the mesh: keep it alive
        self.p = int(p)
        self._h = C.c_void_p()
        kc = None
        if coeff is not None:
            kc = np.ascontiguousarray(coeff, dtype=np.float64).ravel()
            if kc.size != dmesh.counts()[1]:
                raise RuntimeError("Local solver: Input sizes does not match")
        _check(lib().eqlb_primal_create(dmesh._h, C.c_int32(p), _hp(kc) if kc is not None else None,
                                        C.c_int32(MEM_HOST), C.c_void_p(stream), C.byref(self._h)))
        self._read_ndofs()

    @classmethod
    def create_raw(cls, dmesh: DeviceMesh, p: int, coeff=None, memspace=MEM_DEVICE, stream=0):
        """eqlb_primal_create with the coefficient [ncells] behind a raw pointer in `memspace` (None: 1)."""
        self = cls.__new__(cls)
        self.dmesh, self.p, self._h = dmesh, int(p), C.c_void_p()
        _check(lib().eqlb_primal_create(dmesh._h, C.c_int32(p), _vp(coeff), C.c_int32(memspace), C.c_void_p(stream),
                                        C.byref(self._h)))
        self._read_ndofs()
        return self

    def set_dirichlet(self, facets, stream=0):
        """Fixed are the vertex and facet DOFs of the listed facets; a repeated call replaces the mask."""
        fl = np.ascontiguousarray(facets, dtype=np.int32).ravel()
        self.set_dirichlet_raw(fl.size, fl.ctypes.data if fl.size else None, MEM_HOST, stream)

    def set_dirichlet_raw(self, nlist, facets, memspace=MEM_DEVICE, stream=0):
        _check(lib().eqlb_primal_set_dirichlet(self._h, C.c_int32(nlist), _vp(facets), C.c_int32(memspace),
                                               C.c_void_p(stream)))

    def set_diffusion(self, cell_D=None, stream=0):
        """The operator becomes -div(coeff D grad u) (eqlb_primal_set_diffusion): cell_D, a host array [ncells][3] =
        (d00, d01, d11) of the symmetric positive definite tensor of each cell; None switches the term off.  A repeated
        call replaces the tensor; a cell whose values are not finite or not positive definite is refused by name and the
        handle stays as it was.  The diagonal is formed again; Multilevel.set_coarse(True) has to be called again
        afterwards.  D crosses a refinement through Refinement.prolong_dg(0, cell_D.ravel(), bs=3)."""
        kd = None
        if cell_D is not None:
            kd = np.ascontiguousarray(cell_D, dtype=np.float64).ravel()
            if kd.size != 3 * self.dmesh.counts()[1]:
                raise RuntimeError("Local solver: Input sizes does not match")
        self.set_diffusion_raw(None if kd is None else kd.ctypes.data, MEM_HOST, stream)

    def set_diffusion_raw(self, cell_D=None, memspace=MEM_DEVICE, stream=0):
        """cell_D: a raw pointer (int) to [ncells][3] in `memspace`, or None (the term off)."""
        _check(lib().eqlb_primal_set_diffusion(self._h, _vp(cell_D), C.c_int32(memspace), C.c_void_p(stream)))

    def set_robin(self, facets, alpha=1.0, facet_alpha=None, stream=0):
        """The operator gains the boundary mass int alpha u v over the listed boundary facets (eqlb_primal_set_robin):
        -(coeff D grad u) . n = alpha (u - u_ext) there; alpha_f = facet_alpha [nlist] where given, else the scalar.
        An empty list switches the term off; a repeated call replaces the list.  Refused by facet, the handle as it
        was: a facet that is no boundary facet, one listed twice, an alpha that is negative, NaN or infinite.  With some
        alpha_f > 0 the solves no longer ask for a Dirichlet DOF.  The diagonal is formed again;
        Multilevel.set_coarse(True) has to be called again afterwards.  The datum u_ext enters the load through
        lsolver.robin_load; Refinement.carry_robin carries the list to the refined mesh."""
        self._facet_set(facets, [float(alpha)], facet_alpha, stream)

    def robin_list(self):
        """(facets int32 [nlist], facet_alpha [nlist]) as the last accepted set_robin took them (empty without the term).
        Raises for a handle that holds a non-empty list that was not given through set_robin: the host does not know a
        list given through set_robin_raw."""
        return self._facet_list()

    def set_robin_raw(self, nlist, facets, alpha=1.0, facet_alpha=None, memspace=MEM_DEVICE, stream=0):
        """facets int32 [nlist], facet_alpha float64 [nlist] or None behind raw pointers in `memspace`.  Device memory
        space: a listed id that is no boundary facet is skipped; the call waits for the stream.  robin_list() knows
        nothing of a list given here: it is emptied, and Refinement.carry_robin refuses such a handle."""
        self._facet_set_raw(nlist, facets, alpha, facet_alpha, memspace, stream)

    def robin_count(self):
        """The number of listed facets of the Robin term (0 without it)."""
        return self._facet_count()

    def robin_weights(self, stream=0):
        """w_f = alpha_f |E_f| [nlist] in the order of the list (eqlb_primal_robin_weights)."""
        return self._facet_weights(stream)

    def robin_weights_raw(self, w, capacity, memspace=MEM_DEVICE, stream=0):
        return self._facet_weights_raw(w, capacity, memspace, stream)

    def robin_flux(self, u, s, u_ext=None, stream=0):
        """out [nlist, nq] = alpha_i (u_h(x_q) - u_ext[i][q]) on the handle's Robin list at the facet parameters s [nq]
        in the frame of facet_points (eqlb_primal_robin_flux): the point values of the flux condition
        sigma_eq . n that update_flux_bc takes with vector=False.  u_ext [nlist, nq] or None (0)."""
        return self._facet_flux(u, s, u_ext, stream)

    def robin_flux_raw(self, u, s, u_ext, out, memspace=MEM_DEVICE, stream=0):
        """u [ndofs], u_ext [nlist][nq] or None and out [nlist][nq] behind raw pointers in `memspace`; s a host array."""
        self._facet_flux_raw(u, s, u_ext, out, memspace, stream)

    def apply_many(self, U, masked=False, stream=0):
        """Y [nrhs][ndofs]: row c is apply(U[c]), bit for bit, in one call."""
        uu = _columns(U, self.ndofs)
        y = np.zeros_like(uu)
        self.apply_many_raw(uu.shape[0], uu.ctypes.data, y.ctypes.data, masked, MEM_HOST, stream)
        return y

    def apply_many_raw(self, nrhs, u, y, masked=False, memspace=MEM_DEVICE, stream=0):
        _check(lib().eqlb_primal_apply_many(self._h, C.c_int32(nrhs), _vp(u), _vp(y), C.c_int32(1 if masked else 0),
                                            C.c_int32(memspace), C.c_void_p(stream)))

    def solve_many(self, B, U, rtol=1e-8, atol=0.0, maxit=10000, stream=0):
        """nrhs systems in one call: row c of the result and infos[c] are solve(B[c], U[c]), bit for bit.  Returns
        (U, infos)."""
        bb = _columns(B, self.ndofs)
        uu = _columns(U, self.ndofs).copy()
        if uu.shape != bb.shape:
            raise RuntimeError("Local solver: Input sizes does not match")
        infos = self.solve_many_raw(bb.shape[0], bb.ctypes.data, uu.ctypes.data, rtol, atol, maxit, MEM_HOST, stream)
        return uu, infos

    def solve_many_raw(self, nrhs, b, u, rtol=1e-8, atol=0.0, maxit=10000, memspace=MEM_DEVICE, stream=0):
        """eqlb_primal_solve_many on raw pointers: u [nrhs][ndofs] is overwritten by the solutions; waits for the
        device; returns the list of the columns' info."""
        v = (C.c_double * (8 * max(int(nrhs), 1)))()
        _check(lib().eqlb_primal_solve_many(self._h, C.c_int32(nrhs), _vp(b), _vp(u), C.c_double(rtol),
                                            C.c_double(atol), C.c_int32(maxit), v, C.c_int32(memspace),
                                            C.c_void_p(stream)))
        return [_primal_info(v[8 * c:8 * c + 8]) for c in range(int(nrhs))]


class PrimalElasticity(_PrimalSolver):
    """eqlb_elasticity_t: -div(2 eps(u) + pi_1 div(u) I) = f on [P_p]^2 (1 <= p <= 4) with the pi_1 / cell_pi1 convention
    of primal_stress_dg, in the scalar numbering of DeviceMesh.lagrange_dofmap, blocked: x[2 dof + r].  `ndofs` is the
    scalar count; every vector has 2 ndofs rows.  The operator matrix-free, the load vector, the residual and a
    Jacobi-preconditioned CG on the device (lsolver.primal.ElasticityOperator is the numpy statement).  cell_pi1: host
    array [ncells] or None (the scalar everywhere).  Shaped as PrimalPoisson: the methods take and return host arrays;
    the `_raw` variants take raw pointers (ints) in `memspace`, ordered on `stream`."""

    _prefix, _bs = "eqlb_elasticity_", 2
    _facet = ("set_springs", "spring", 3)

    def __init__(self, dmesh: DeviceMesh, p: int, pi_1: float = 1.0, cell_pi1=None, stream=0):
        self.dmesh = dmesh   # the handle reads the mesh: keep it alive
        self.p = int(p)
        self._h = C.c_void_p()
        kc = None
        if cell_pi1 is not None:
            kc = np.ascontiguousarray(cell_pi1, dtype=np.float64).ravel()
            if kc.size != dmesh.counts()[1]:
                raise RuntimeError("Local solver: Input sizes does not match")
        _check(lib().eqlb_elasticity_create(dmesh._h, C.c_int32(p), C.c_double(pi_1),
                                            _hp(kc) if kc is not None else None, C.c_int32(MEM_HOST),
                                            C.c_void_p(stream), C.byref(self._h)))
        self._read_ndofs()

    @classmethod
    def create_raw(cls, dmesh: DeviceMesh, p: int, pi_1: float = 1.0, cell_pi1=None, memspace=MEM_DEVICE, stream=0):
        """eqlb_elasticity_create with cell_pi1 [ncells] behind a raw pointer in `memspace` (None: the scalar)."""
        self = cls.__new__(cls)
        self.dmesh, self.p, self._h = dmesh, int(p), C.c_void_p()
        _check(lib().eqlb_elasticity_create(dmesh._h, C.c_int32(p), C.c_double(pi_1), _vp(cell_pi1),
                                            C.c_int32(memspace), C.c_void_p(stream), C.byref(self._h)))
        self._read_ndofs()
        return self

    def set_dirichlet(self, facets0, facets1, stream=0):
        """Fixed are the rows 2 dof + r of the vertex and facet DOFs of the facets listed for component r (the facets
        with type 1 in row r of a stress handle); a repeated call replaces the mask."""
        f0 = np.ascontiguousarray(facets0, dtype=np.int32).ravel()
        f1 = np.ascontiguousarray(facets1, dtype=np.int32).ravel()
        self.set_dirichlet_raw(f0.size, f0.ctypes.data if f0.size else None, f1.size,
                               f1.ctypes.data if f1.size else None, MEM_HOST, stream)

    def set_dirichlet_raw(self, nlist0, facets0, nlist1, facets1, memspace=MEM_DEVICE, stream=0):
        _check(lib().eqlb_elasticity_set_dirichlet(self._h, C.c_int32(nlist0), _vp(facets0), C.c_int32(nlist1),
                                                   _vp(facets1), C.c_int32(memspace), C.c_void_p(stream)))

    def set_shear(self, mu=1.0, cell_mu=None, stream=0):
        """The stress becomes mu (2 eps(u) + pi_1 div(u) I) (eqlb_elasticity_set_shear): cell_mu, a host array [ncells],
        where given, else the scalar mu on every cell, mu > 0; mu == 1 without an array switches the term off.  The
        reaction term is not scaled.  A repeated call replaces the coefficient; one that is <= 0, NaN or infinite is
        refused, the cell named, and the handle stays as it was.  The diagonal is formed again;
        Multilevel.set_coarse(True) has to be called again afterwards.  A DG_0 coefficient crosses a refinement through
        Refinement.prolong_dg(0, cell_mu): the children of a cell take its value."""
        kc = None
        if cell_mu is not None:
            kc = np.ascontiguousarray(cell_mu, dtype=np.float64).ravel()
            if kc.size != self.dmesh.counts()[1]:
                raise RuntimeError("Local solver: Input sizes does not match")
        self.set_shear_raw(mu, None if kc is None else kc.ctypes.data, MEM_HOST, stream)

    def set_shear_raw(self, mu=1.0, cell_mu=None, memspace=MEM_DEVICE, stream=0):
        """cell_mu: a raw pointer (int) to [ncells] in `memspace`, or None (the scalar mu)."""
        _check(lib().eqlb_elasticity_set_shear(self._h, C.c_double(mu), _vp(cell_mu), C.c_int32(memspace),
                                               C.c_void_p(stream)))

    def set_springs(self, facets, k=1.0, facet_k=None, stream=0):
        """The operator gains int_E v^T K u over the listed boundary facets (eqlb_elasticity_set_springs):
        sigma(u) n = -K (u - u_ext) there; K_f = facet_k [nlist, 3] = (k00, k01, k11), symmetric positive semidefinite
        in global axes, where given, else k I.  An empty list switches the term off; a repeated call replaces the list.
        Refused by facet, the handle as it was: a facet that is no boundary facet, one listed twice, an entry that is
        not finite, k00 < 0, k11 < 0, k01 k01 > k00 k11 (1 + 2^-49).  With a positive definite K_f on some facet the
        solves ask for no Dirichlet DOF.  The diagonal is formed again; Multilevel.set_coarse(True) has to be called
        again afterwards.  The datum u_ext enters the load through lsolver.spring_load; lsolver.spring_tensor gives
        K = kn n x n + kt t x t; Refinement.carry_springs carries the list to the refined mesh."""
        self._facet_set(facets, [float(k), 0.0, float(k)], facet_k, stream)

    def spring_list(self):
        """(facets int32 [nlist], facet_k [nlist, 3]) as the last accepted set_springs took them (empty without the
        term).  Raises for a handle that holds a non-empty list that was not given through set_springs."""
        return self._facet_list()

    def set_springs_raw(self, nlist, facets, k=1.0, facet_k=None, memspace=MEM_DEVICE, stream=0):
        """facets int32 [nlist], facet_k float64 [nlist][3] or None behind raw pointers in `memspace`.  Device memory
        space: a listed id that is no boundary facet is skipped; the call waits for the stream.  spring_list() knows
        nothing of a list given here: it is emptied, and Refinement.carry_springs refuses such a handle."""
        self._facet_set_raw(nlist, facets, k, facet_k, memspace, stream)

    def spring_count(self):
        """The number of listed facets of the spring term (0 without it)."""
        return self._facet_count()

    def spring_weights(self, stream=0):
        """Kw_f = |E_f| (k00, k01, k11) [nlist, 3] in the order of the list (eqlb_elasticity_spring_weights)."""
        return self._facet_weights(stream)

    def spring_weights_raw(self, kw, capacity, memspace=MEM_DEVICE, stream=0):
        return self._facet_weights_raw(kw, capacity, memspace, stream)

    def spring_flux(self, u, s, u_ext=None, stream=0):
        """out [2, nlist, nq]: out[r] = (K (u_h - u_ext))_r on the handle's spring list at the facet parameters s [nq] in
        the frame of facet_points (eqlb_elasticity_spring_flux): row r holds the point values of the flux condition that
        row r of a stress handle takes in update_flux_bc with vector=False.  u_ext [2, nlist, nq] or None (0)."""
        return self._facet_flux(u, s, u_ext, stream)

    def spring_flux_raw(self, u, s, u_ext, out, memspace=MEM_DEVICE, stream=0):
        """u [2 ndofs], u_ext [2][nlist][nq] or None and out [2][nlist][nq] behind raw pointers in `memspace`; s a host
        array."""
        self._facet_flux_raw(u, s, u_ext, out, memspace, stream)


class Multilevel:
    """eqlb_hierarchy_t: the multilevel preconditioner (additive multilevel diagonal scaling, BPX) of the P_p solves over
    the levels of an adaptive loop, and the CG of the finest handle with it (lsolver.multilevel.Hierarchy is the numpy
    statement).  solvers: PrimalPoisson handles, or PrimalElasticity handles, coarsest first, all of one p;
    refinements[l]: the Refinement of DeviceMesh.refine(..., keep_plan=True) from the mesh of solvers[l] to that of
    solvers[l + 1].  Everything is borrowed (and kept alive here); masks and diagonals are read when a call runs, so
    set_dirichlet on a level takes effect at the next call.  One level is plain Jacobi.  The methods take and return host
    arrays; the `_raw` variants take raw pointers (ints) in `memspace`, ordered on `stream`.  The calls use the work
    space of the solver handles: one stream, one call after the other.
    local=True (or the `local` property, at any time): local smoothing for adaptively refined hierarchies - a level
    l >= 1 smooths only the rows whose basis function is new or changed there (Hierarchy(..., local=True) states the
    rule); precondition, solve and their _many forms honour it.  active(level) / active_count(level) show the rows.
    coarse=True (or the `coarse` property, at any time): level 0 is solved exactly on its free rows (at most 4096) by a
    dense LDL^T factor in the place of its diagonal (Hierarchy(..., coarse=True) states the rule).  The factor is a
    snapshot of the mask and the coefficient of level 0: every set_coarse(True) factors again, and set_dirichlet or a
    new coefficient on level 0 needs another one.  coarse_rows / coarse_factor() show it."""

    def __init__(self, solvers, refinements, local=False, stream=0, coarse=False):
        self.solvers, self.refinements = list(solvers), list(refinements)
        self._h = C.c_void_p()
        self._local = False
        self._coarse = False
        n = len(self.solvers)
        if n < 1 or len(self.refinements) != n - 1:
            raise RuntimeError("Multilevel: one Refinement per pair of neighbouring levels expected")
        el = [isinstance(s, PrimalElasticity) for s in self.solvers]
        if any(el) != all(el) or not all(isinstance(s, (PrimalPoisson, PrimalElasticity)) for s in self.solvers):
            raise RuntimeError("Multilevel: PrimalPoisson handles or PrimalElasticity handles expected, not a mixture")
        self.bs = 2 if el[0] else 1
        plans = [r._kept_plan("Multilevel") for r in self.refinements]
        self.nrows = [self.bs * s.ndofs for s in self.solvers]
        sv = (C.c_void_p * n)(*[s._h.value for s in self.solvers])
        ms = (C.c_void_p * n)(*[s.dmesh._h.value for s in self.solvers])
        pl = (C.c_void_p * max(n - 1, 1))(*[q._h.value for q in plans])
        _check(lib().eqlb_hierarchy_create(C.c_int32(n), C.c_int32(self.bs), sv, pl, ms, C.c_void_p(stream),
                                           C.byref(self._h)))
        if local:
            self.set_local(True, stream)
        if coarse:
            self.set_coarse(True, stream)

    @property
    def nlevels(self):
        return len(self.solvers)

    @property
    def local(self):
        return self._local

    @local.setter
    def local(self, on):
        self.set_local(on)

    def set_local(self, on, stream=0):
        """eqlb_hierarchy_set_local: switching on writes the masks on `stream` and waits for the device."""
        flag = int(on) if isinstance(on, (bool, int, np.integer)) else -1
        _check(lib().eqlb_hierarchy_set_local(self._h, C.c_int32(flag), C.c_void_p(stream)))
        self._local = bool(flag)

    def active(self, level, stream=0):
        """bool [bs * ndofs_level]: the rows the local rule smooths on `level` (all of level 0)."""
        ok = 0 <= level < self.nlevels
        out = np.zeros(self.nrows[level] if ok else 1, dtype=np.uint8)
        self.active_raw(level, out.ctypes.data, out.size, MEM_HOST, stream)
        return out.astype(bool)

    def active_raw(self, level, out, capacity, memspace=MEM_DEVICE, stream=0):
        _check(lib().eqlb_hierarchy_active(self._h, C.c_int32(level), _vp(out), C.c_int64(capacity),
                                           C.c_int32(memspace), C.c_void_p(stream)))

    def active_count(self, level):
        n = C.c_int64(0)
        _check(lib().eqlb_hierarchy_active_count(self._h, C.c_int32(level), C.byref(n)))
        return int(n.value)

    @property
    def coarse(self):
        return self._coarse

    @coarse.setter
    def coarse(self, on):
        self.set_coarse(on)

    def set_coarse(self, on, stream=0):
        """eqlb_hierarchy_set_coarse: switching on factors level 0 on `stream` (again, if it was on) and waits for the
        device; a refusal leaves the switch off."""
        flag = int(on) if isinstance(on, (bool, int, np.integer)) else -1
        if flag == 1:
            self._coarse = False
        _check(lib().eqlb_hierarchy_set_coarse(self._h, C.c_int32(flag), C.c_void_p(stream)))
        self._coarse = bool(flag)

    @property
    def coarse_rows(self):
        """the number of free rows of level 0 the factor was formed on"""
        n = C.c_int64(0)
        _check(lib().eqlb_hierarchy_coarse_rows(self._h, C.byref(n)))
        return int(n.value)

    def coarse_factor(self, stream=0):
        """(rows int32 [n], d [n], W [n][n]): the free rows of level 0, the pivots and the unit lower triangular
        W = L^-1 of the factor."""
        n = self.coarse_rows
        rows, d, W = np.zeros(n, dtype=np.int32), np.zeros(n), np.zeros((n, n))
        self.coarse_factor_raw(rows.ctypes.data, d.ctypes.data, W.ctypes.data, n, MEM_HOST, stream)
        return rows, d, W

    def coarse_factor_raw(self, rows, d, W, capacity, memspace=MEM_DEVICE, stream=0):
        _check(lib().eqlb_hierarchy_coarse_factor(self._h, _vp(rows), _vp(d), _vp(W), C.c_int64(capacity),
                                                  C.c_int32(memspace), C.c_void_p(stream)))

    def _vec(self, a, level):
        v = np.ascontiguousarray(a, dtype=np.float64).ravel()
        if v.size != self.nrows[level]:
            raise RuntimeError("Local solver: Input sizes does not match")
        return v

    def restrict(self, level, r, masked=True, stream=0):
        """r of level + 1 -> P^T r of `level` (the transpose of Refinement.prolong); masked: 0 on the fixed rows of
        `level`."""
        ok = 0 <= level < self.nlevels - 1
        rr = self._vec(r, level + 1) if ok else np.ascontiguousarray(r, dtype=np.float64).ravel()
        out = np.zeros(self.nrows[level] if ok else 1)
        self.restrict_raw(level, rr.ctypes.data, out.ctypes.data, masked, MEM_HOST, stream)
        return out

    def restrict_raw(self, level, r_fine, r_coarse, masked=True, memspace=MEM_DEVICE, stream=0):
        _check(lib().eqlb_hierarchy_restrict(self._h, C.c_int32(level), _vp(r_fine), _vp(r_coarse),
                                             C.c_int32(1 if masked else 0), C.c_int32(memspace), C.c_void_p(stream)))

    def precondition(self, r, stream=0):
        """z = M r on the finest level."""
        rr, z = self._vec(r, -1), np.zeros(self.nrows[-1])
        self.precondition_raw(rr.ctypes.data, z.ctypes.data, MEM_HOST, stream)
        return z

    def precondition_raw(self, r, z, memspace=MEM_DEVICE, stream=0):
        _check(lib().eqlb_hierarchy_precondition(self._h, _vp(r), _vp(z), C.c_int32(memspace), C.c_void_p(stream)))

    def solve(self, b, u, rtol=1e-8, atol=0.0, maxit=10000, stream=0):
        """The CG of the finest handle with the multilevel preconditioner, from the start u (its fixed rows hold the
        Dirichlet values).  Returns (u, info) as PrimalPoisson.solve; breakdown also reports r . z <= 0."""
        bb = self._vec(b, -1)
        uu = self._vec(u, -1).copy()
        info = self.solve_raw(bb.ctypes.data, uu.ctypes.data, rtol, atol, maxit, MEM_HOST, stream)
        return uu, info

    def solve_raw(self, b, u, rtol=1e-8, atol=0.0, maxit=10000, memspace=MEM_DEVICE, stream=0):
        """eqlb_hierarchy_solve on raw pointers: u is overwritten by the solution; waits for the device; returns info."""
        v = (C.c_double * 8)()
        _check(lib().eqlb_hierarchy_solve(self._h, _vp(b), _vp(u), C.c_double(rtol), C.c_double(atol), C.c_int32(maxit),
                                          v, C.c_int32(memspace), C.c_void_p(stream)))
        info = dict(zip(PRIMAL_INFO, [float(x) for x in v]))
        for key in ("iterations", "converged", "replacements", "breakdown", "facets_skipped"):
            info[key] = int(info[key])
        return info

    def precondition_many(self, R, stream=0):
        """Z [nrhs][n]: row c is precondition(R[c]), bit for bit, in one call (Poisson handles only)."""
        rr = _columns(R, self.nrows[-1])
        z = np.zeros_like(rr)
        self.precondition_many_raw(rr.shape[0], rr.ctypes.data, z.ctypes.data, MEM_HOST, stream)
        return z

    def precondition_many_raw(self, nrhs, r, z, memspace=MEM_DEVICE, stream=0):
        _check(lib().eqlb_hierarchy_precondition_many(self._h, C.c_int32(nrhs), _vp(r), _vp(z), C.c_int32(memspace),
                                                      C.c_void_p(stream)))

    def solve_many(self, B, U, rtol=1e-8, atol=0.0, maxit=10000, stream=0):
        """nrhs systems in one call: row c of the result and infos[c] are solve(B[c], U[c]), bit for bit (Poisson
        handles only).  Returns (U, infos)."""
        bb = _columns(B, self.nrows[-1])
        uu = _columns(U, self.nrows[-1]).copy()
        if uu.shape != bb.shape:
            raise RuntimeError("Local solver: Input sizes does not match")
        infos = self.solve_many_raw(bb.shape[0], bb.ctypes.data, uu.ctypes.data, rtol, atol, maxit, MEM_HOST, stream)
        return uu, infos

    def solve_many_raw(self, nrhs, b, u, rtol=1e-8, atol=0.0, maxit=10000, memspace=MEM_DEVICE, stream=0):
        """eqlb_hierarchy_solve_many on raw pointers: u [nrhs][n] is overwritten by the solutions; waits for the
        device; returns the list of the columns' info."""
        v = (C.c_double * (8 * max(int(nrhs), 1)))()
        _check(lib().eqlb_hierarchy_solve_many(self._h, C.c_int32(nrhs), _vp(b), _vp(u), C.c_double(rtol),
                                               C.c_double(atol), C.c_int32(maxit), v, C.c_int32(memspace),
                                               C.c_void_p(stream)))
        return [_primal_info(v[8 * c:8 * c + 8]) for c in range(int(nrhs))]

    def close(self):
        if self._h:
            lib().eqlb_hierarchy_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def halo_pack(x_ptr, cells_ptr, buf_ptr, nrhs, nlist, nrt, ncells, clear=True, stream=0):
    """eqlb_halo_pack on raw device pointers (asynchronous on `stream`)."""
    _check(lib().eqlb_halo_pack(C.c_int32(nrhs), C.c_int32(nlist), C.c_int32(nrt), C.c_int64(ncells),
                                C.c_void_p(cells_ptr), C.c_void_p(x_ptr), C.c_void_p(buf_ptr),
                                C.c_int32(int(clear)), C.c_void_p(stream)))


def halo_unpack_add(x_ptr, cells_ptr, buf_ptr, nrhs, nlist, nrt, ncells, stream=0):
    _check(lib().eqlb_halo_unpack_add(C.c_int32(nrhs), C.c_int32(nlist), C.c_int32(nrt),
                                      C.c_int64(ncells), C.c_void_p(cells_ptr), C.c_void_p(x_ptr),
                                      C.c_void_p(buf_ptr), C.c_void_p(stream)))


class RcclComm:
    """An RCCL communicator made through the library (eqlb_rccl_get_unique_id / eqlb_rccl_comm_create): what
    a host without an RCCL binding of its own uses for eqlb_halo_exchange / eqlb_halo_reduce.  The 128-byte
    unique id is made on one rank (`RcclComm.unique_id()`) and distributed by the caller."""

    def __init__(self, unique_id: bytes, nranks: int, rank: int):
        if len(unique_id) != 128:
            raise RuntimeError("RcclComm: the unique id has 128 bytes")
        self._h = C.c_void_p()
        buf = C.create_string_buffer(bytes(unique_id), 128)
        _check(lib().eqlb_rccl_comm_create(buf, C.c_int32(nranks), C.c_int32(rank), C.byref(self._h)))
        self.nranks, self.rank = nranks, rank

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        _check(lib().eqlb_rccl_get_unique_id(buf))
        return buf.raw

    @property
    def handle(self):
        return self._h.value

    def destroy(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().eqlb_rccl_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class HaloPlan:
    """Host-side argument block of eqlb_halo_reduce / eqlb_halo_exchange: peers and, per peer, device index
    lists and device staging buffers (raw pointers; the caller keeps the memory alive)."""

    def __init__(self, peers, send_idx_ptrs, nsend, send_buf_ptrs, recv_idx_ptrs, nrecv, recv_buf_ptrs):
        n = len(peers)
        self.n = n
        self.peers = (C.c_int32 * n)(*[int(q) for q in peers])
        self.send_idx = (C.c_void_p * n)(*[C.c_void_p(int(p) or None) for p in send_idx_ptrs])
        self.recv_idx = (C.c_void_p * n)(*[C.c_void_p(int(p) or None) for p in recv_idx_ptrs])
        self.send_buf = (C.c_void_p * n)(*[C.c_void_p(int(p) or None) for p in send_buf_ptrs])
        self.recv_buf = (C.c_void_p * n)(*[C.c_void_p(int(p) or None) for p in recv_buf_ptrs])
        self.nsend = (C.c_int64 * n)(*[int(v) for v in nsend])
        self.nrecv = (C.c_int64 * n)(*[int(v) for v in nrecv])


def halo_reduce(comm, plan: HaloPlan, x_ptr, nrhs, nrt, nentries, stream=0):
    """eqlb_halo_reduce: pack (+ clear), grouped RCCL send / recv, unpack-add - one call, asynchronous."""
    h = comm.handle if isinstance(comm, RcclComm) else comm
    _check(lib().eqlb_halo_reduce(C.c_void_p(h), C.c_int32(nrhs), C.c_int32(nrt), C.c_int64(nentries),
                                  C.c_void_p(x_ptr), C.c_int32(plan.n), plan.peers, plan.send_idx, plan.nsend,
                                  plan.send_buf, plan.recv_idx, plan.nrecv, plan.recv_buf, C.c_void_p(stream)))


def halo_exchange(comm, plan: HaloPlan, nrhs, nrt, stream=0):
    """eqlb_halo_exchange: the grouped send / recv alone (between halo_pack and halo_unpack_add)."""
    h = comm.handle if isinstance(comm, RcclComm) else comm
    sc = (C.c_int64 * plan.n)(*[int(v) * nrhs * nrt for v in plan.nsend])
    rc = (C.c_int64 * plan.n)(*[int(v) * nrhs * nrt for v in plan.nrecv])
    _check(lib().eqlb_halo_exchange(C.c_void_p(h), C.c_int32(plan.n), plan.peers, plan.send_buf, sc,
                                    plan.recv_buf, rc, C.c_void_p(stream)))


def get_reference_table(k, degree_dg, name):
    nrt, nd, nq = k * (k + 2), (degree_dg + 1) * (degree_dg + 2) // 2, k * (k + 1) // 2
    shapes = {"S": (3, nrt, nrt), "F": (3, 3, nd, k), "H": (3, nd, nq), "D": (3, nd, 2, nq)}
    out = np.zeros(shapes[name])
    n = lib().eqlb_get_reference_table(C.c_int32(k), C.c_int32(degree_dg), name.encode(),
                                       _hp(out), C.c_int32(out.size))
    if n != out.size:
        raise RuntimeError(lib().eqlb_last_error().decode())
    return out


def reconstruct_fluxes_semiexplt(flux_hdiv, flux_dg, rhs_dg, boundary_data, reconstruct_stress):
    """Same name and argument order as the reference binding (wrappers.cpp:97-115); the
    arguments are flat arrays [nrhs, ...] and `boundary_data` is a configured
    SemiExplicitEquilibrator (it carries the facet types like base::BoundaryData does)."""
    if bool(reconstruct_stress) != bool(getattr(boundary_data, "reconstruct_stress", False)):
        raise RuntimeError("reconstruct_stress does not match the equilibrator handle")
    return boundary_data.equilibrate_host(flux_dg, rhs_dg, flux_hdiv)
