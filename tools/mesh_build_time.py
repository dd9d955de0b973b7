"""Time of a mesh handle at 1M triangles, median of 5 after one warm-up run each:
  (a) create_mesh on the host (numpy)                      - what a caller of (b) pays before it
  (b) DeviceMesh(mesh): eqlb_mesh_create from the finished arrays
  (c) DeviceMesh.from_cells from host arrays               - C call and the export into .mesh; the C call alone as well
  (d) DeviceMesh.from_cells from device arrays (torch)
and the phases of the C call of (c) as the library reports them with EQLB_PROFILE_SETUP=1 (each phase closed by a
synchronisation of its own, so their sum is a little above the plain call)."""
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from dolfinx_eqlb_amd import cpp
from dolfinx_eqlb_amd import distributed as dd
from dolfinx_eqlb_amd.mesh import create_mesh

REPEAT = 5


def median_ms(fn):
    fn()
    times = []
    for _ in range(REPEAT):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keep = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        del keep
    return statistics.median(times)


def c_call(x, cells):
    h = C.c_void_p()
    st = cpp.lib().eqlb_mesh_create_from_cells(C.c_int32(x.shape[0]), C.c_int32(cells.shape[0]),
                                               x.ctypes.data_as(C.c_void_p), cells.ctypes.data_as(C.c_void_p),
                                               C.c_int32(cpp.MEM_HOST), None, C.byref(h))
    assert st == 0, cpp.lib().eqlb_last_error().decode()
    cpp.lib().eqlb_mesh_destroy(h)


torch.cuda.init()
mesh = dd.StripPartition(500, 0, 1).mesh
x = np.ascontiguousarray(mesh.x)
cells = np.ascontiguousarray(mesh.cell_nodes)
print("%d cells, %d nodes, %d facets" % (mesh.ncells, mesh.nnodes, mesh.nfacets))
t_a = median_ms(lambda: create_mesh(x[:, :2], cells))
t_b = median_ms(lambda: cpp.DeviceMesh(mesh))
t_c = median_ms(lambda: cpp.DeviceMesh.from_cells(x, cells))
t_cc = median_ms(lambda: c_call(x, cells))
dx, dc = torch.from_numpy(x).to("cuda"), torch.from_numpy(cells).to("cuda")
st = torch.cuda.current_stream().cuda_stream
t_d = median_ms(lambda: cpp.DeviceMesh.from_cells(dx, dc, device=True, stream=st))
print("(a) create_mesh on the host            %8.1f ms" % t_a)
print("(b) DeviceMesh(mesh), finished arrays  %8.1f ms" % t_b)
print("(c) DeviceMesh.from_cells, host arrays %8.1f ms   (eqlb_mesh_create_from_cells alone %.1f ms)" % (t_c, t_cc))
print("(d) DeviceMesh.from_cells, device      %8.1f ms" % t_d)
print("(c) <= (b): %s" % ("yes" if t_c <= t_b else "NO"))
sys.stdout.flush()
os.environ["EQLB_PROFILE_SETUP"] = "1"
c_call(x, cells)
