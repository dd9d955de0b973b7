"""Time of one refinement step at 1M triangles (crossed 500 x 500), median of 5 after one warm-up run each, with a
device synchronisation on either side.  The marked list comes from eqlb_mark_doerfler on lognormal(0, 2) indicators at
theta = 0.5 (the input of tools/bench_marking.py, about 2 % of the cells) and lies in device memory.
  (a) the device route: eqlb_mesh_refine_plan + eqlb_refine_create_mesh + eqlb_refine_parent_facets from device arrays
  (b) the host route: the numpy statement mesh.refine.refine_longest_edge + DeviceMesh.from_cells from host arrays +
      the statement's parent_facets
and the parts of (a): the plan (closure, scans and the one wait), the write of all four outputs into device arrays,
the mesh build (also alone, and on the unrefined mesh), the parent facets.  The phases of the plan and of the mesh
build follow as the library reports them with EQLB_PROFILE_SETUP=1 (each phase closed by a synchronisation of its own, so their sum is a little above the plain call)."""
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from dolfinx_eqlb_amd import cpp
from dolfinx_eqlb_amd.mesh import create_unit_square, parent_facets, refine_longest_edge

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


torch.cuda.init()
st = torch.cuda.current_stream().cuda_stream
mesh = create_unit_square(500)
n = mesh.ncells
dm = cpp.DeviceMesh.from_cells(mesh.x, mesh.cell_nodes)
eta = torch.from_numpy(np.random.default_rng(0).lognormal(0, 2, n)).to("cuda")
marked = torch.empty(n, dtype=torch.int32, device="cuda")
nmarked = torch.zeros(1, dtype=torch.int64, device="cuda")
cpp.mark_doerfler_raw(n, eta.data_ptr(), 0.5, marked.data_ptr(), nmarked.data_ptr(), None, cpp.MEM_DEVICE, st)
torch.cuda.synchronize()
nm = int(nmarked.item())
ids = marked[:nm].cpu().numpy()


def plan():
    return dm.refine_raw(marked.data_ptr(), nmarked.data_ptr(), n, cpp.MEM_DEVICE, st)


def c_build(dx, dc):
    """eqlb_mesh_create_from_cells alone on device arrays."""
    h = C.c_void_p()
    s_ = cpp.lib().eqlb_mesh_create_from_cells(C.c_int32(dx.shape[0]), C.c_int32(dc.shape[0]), C.c_void_p(dx.data_ptr()),
                                               C.c_void_p(dc.data_ptr()), C.c_int32(cpp.MEM_DEVICE), C.c_void_p(st),
                                               C.byref(h))
    assert s_ == 0, cpp.lib().eqlb_last_error().decode()
    cpp.lib().eqlb_mesh_destroy(h)


p = plan()
nn2, nc2, nbis, ncut = p.counts()
new = p.create_mesh(st)
nf2 = new.counts()[2]
print("%d cells, %d marked -> %d cells cut, %d facets bisected, %d cells, %d nodes, %d facets"
      % (n, nm, ncut, nbis, nc2, nn2, nf2))
d_x = torch.empty((nn2, 3), dtype=torch.float64, device="cuda")
d_c = torch.empty((nc2, 3), dtype=torch.int32, device="cuda")
d_pc = torch.empty(nc2, dtype=torch.int32, device="cuda")
d_npf = torch.empty(nbis, dtype=torch.int32, device="cuda")
d_pf = torch.empty(nf2, dtype=torch.int32, device="cuda")


def device_route():
    q = plan()
    m2 = q.create_mesh(st)
    q.parent_facets_raw(m2, d_pf.data_ptr(), cpp.MEM_DEVICE, st)
    torch.cuda.synchronize()   # the plan is destroyed on return
    return m2


def host_route():
    x2, c2, pc, npf = refine_longest_edge(mesh, ids)
    m2 = cpp.DeviceMesh.from_cells(x2, c2)
    return m2, parent_facets(mesh, npf, m2.mesh)


t_a = median_ms(device_route)
t_plan = median_ms(plan)
t_write = median_ms(lambda: p.write_raw(d_x.data_ptr(), d_c.data_ptr(), d_pc.data_ptr(), d_npf.data_ptr(),
                                        cpp.MEM_DEVICE, st))
t_mesh = median_ms(lambda: p.create_mesh(st))
t_build = median_ms(lambda: c_build(d_x, d_c))
d_x0, d_c0 = torch.from_numpy(mesh.x).to("cuda"), torch.from_numpy(mesh.cell_nodes).to("cuda")
t_build0 = median_ms(lambda: c_build(d_x0, d_c0))
t_pf = median_ms(lambda: p.parent_facets_raw(new, d_pf.data_ptr(), cpp.MEM_DEVICE, st))
t_stmt = median_ms(lambda: refine_longest_edge(mesh, ids))
t_b = median_ms(host_route)
x2_h, c2_h, _, npf_h = refine_longest_edge(mesh, ids)
t_fc = median_ms(lambda: cpp.DeviceMesh.from_cells(x2_h, c2_h))
m2, pf = host_route()
same = np.array_equal(m2.mesh.x, d_x.cpu().numpy()) and np.array_equal(m2.mesh.cell_nodes, d_c.cpu().numpy()) \
    and np.array_equal(pf, d_pf.cpu().numpy())
print("(a) device route: plan + create_mesh + parent_facets %8.1f ms" % t_a)
print("      plan (closure, scans, one wait)                %8.2f ms" % t_plan)
print("      write of the four outputs, device arrays       %8.2f ms" % t_write)
print("      create_mesh (write of x2, cells + mesh build)  %8.2f ms" % t_mesh)
print("        eqlb_mesh_create_from_cells alone on them    %8.2f ms   (with eqlb_mesh_destroy)" % t_build)
print("        the same call on the unrefined mesh          %8.2f ms" % t_build0)
print("      parent_facets                                  %8.2f ms" % t_pf)
print("(b) host route: statement + from_cells + parents     %8.1f ms   (refine_longest_edge alone %.1f ms, "
      "DeviceMesh.from_cells alone %.1f ms)" % (t_b, t_stmt, t_fc))
print("(a) and (b) give the same mesh and parent facets: %s" % ("yes" if same else "NO"))
sys.stdout.flush()
os.environ["EQLB_PROFILE_SETUP"] = "1"
plan().create_mesh(st)
