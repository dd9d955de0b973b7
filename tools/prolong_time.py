"""Time of the transfer across one refinement step at 1M triangles (crossed 500 x 500, the mesh and the marked list of
tools/refine_time.py: eqlb_mark_doerfler on lognormal(0, 2) indicators at theta = 0.5, about 2 % of the cells), median
of 5 after one warm-up run each, with a device synchronisation on either side.  Three transfers:
  P_2  u_h          [1][ndofs]            eqlb_refine_prolong_lagrange, dofmaps of eqlb_mesh_lagrange_dofmap
  DG_1 flux         [1][ncells*3*2]       eqlb_refine_prolong_dg, bs = 2
  DG_0 coefficient  [1][ncells]           eqlb_refine_prolong_dg
each on two routes:
  (a) device: the data lies in device memory and stays there; one kernel on the stream
  (b) host:   the numpy statement of dolfinx_eqlb_amd.mesh.transfer on host arrays, then the upload of the result
              (what a caller without these entries does; the download of u_h that precedes it is not counted)
and, next to them, the two device dofmaps and the bytes each kernel has to move at the least (inputs read once, outputs
written once, the index tables it walks), as a rate over the measured time.  The host side depends on the CPU."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from dolfinx_eqlb_amd import cpp
from dolfinx_eqlb_amd.mesh import create_unit_square, prolong_dg, prolong_lagrange

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
r = dm.refine((marked, nmarked), device=True, stream=st, keep_plan=True)
mesh2 = r.dmesh.mesh
n2 = mesh2.ncells
pc, npf = r.parent_cell.cpu().numpy(), r.node_parent_facet.cpu().numpy()
print("%d cells, %d marked -> %d cells, %d nodes" % (n, int(nmarked.item()), n2, mesh2.nnodes))

P, D = 2, 1
d_cd, ndofs = dm.lagrange_dofmap(P, device=True, stream=st)
d_cd2, ndofs2 = r.dmesh.lagrange_dofmap(P, device=True, stream=st)
torch.cuda.synchronize()
cd, cd2 = d_cd.cpu().numpy(), d_cd2.cpu().numpy()
rng = np.random.default_rng(1)
u = rng.standard_normal((1, ndofs))
flux = rng.standard_normal((1, n * 3 * 2))
coeff = rng.lognormal(0, 1, (1, n))
d_u, d_flux, d_coeff = [torch.from_numpy(a).to("cuda") for a in (u, flux, coeff)]
d_u2 = torch.zeros((1, ndofs2), dtype=torch.float64, device="cuda")
d_flux2 = torch.empty((1, n2 * 3 * 2), dtype=torch.float64, device="cuda")
d_coeff2 = torch.empty((1, n2), dtype=torch.float64, device="cuda")
plan = r.plan


def dev_u():
    plan.prolong_lagrange_raw(r.dmesh, P, 1, 1, d_cd.data_ptr(), ndofs, d_u.data_ptr(), d_cd2.data_ptr(), ndofs2,
                              d_u2.data_ptr(), cpp.MEM_DEVICE, st)


def dev_flux():
    plan.prolong_dg_raw(r.dmesh, D, 2, 1, d_flux.data_ptr(), d_flux2.data_ptr(), cpp.MEM_DEVICE, st)


def dev_coeff():
    plan.prolong_dg_raw(r.dmesh, 0, 1, 1, d_coeff.data_ptr(), d_coeff2.data_ptr(), cpp.MEM_DEVICE, st)


def host_u():
    return torch.from_numpy(prolong_lagrange(mesh, mesh2, pc, npf, P, u, cell_dofs=cd, cell_dofs2=cd2,
                                             ndofs2=ndofs2)).to("cuda")


def host_flux():
    return torch.from_numpy(prolong_dg(mesh, mesh2, pc, npf, D, flux, bs=2)).to("cuda")


def host_coeff():
    return torch.from_numpy(prolong_dg(mesh, mesh2, pc, npf, 0, coeff)).to("cuda")


# least traffic: the cells of both meshes (12 B each), the child offsets, the data in and out, and for P_2 the two
# dofmaps (24 B per cell) and the owner look-ups (node -> cell and facet -> cell: two 4-byte reads per vertex and facet)
walk = 12 * n + 4 * n + 12 * n2
bytes_u = walk + 24 * (n + n2) + 8 * (ndofs + ndofs2) + 12 * n2 + 8 * 6 * n2
bytes_flux = walk + 8 * 6 * (n + n2)
bytes_coeff = 4 * n + 8 * (n + n2)
same = []
rows = []
for name, dev, host, out, nbytes in (("P_2 u_h", dev_u, host_u, d_u2, bytes_u),
                                     ("DG_1 flux (bs = 2)", dev_flux, host_flux, d_flux2, bytes_flux),
                                     ("DG_0 coefficient", dev_coeff, host_coeff, d_coeff2, bytes_coeff)):
    t_d, t_h = median_ms(dev), median_ms(host)
    same.append(bool(torch.equal(out, host())))
    rows.append((name, t_d, t_h, nbytes))
t_map = median_ms(lambda: dm.lagrange_dofmap_raw(P, d_cd.data_ptr(), cpp.MEM_DEVICE, st))
t_map2 = median_ms(lambda: r.dmesh.lagrange_dofmap_raw(P, d_cd2.data_ptr(), cpp.MEM_DEVICE, st))
for name, t_d, t_h, nbytes in rows:
    print("%-20s (a) device %8.3f ms  (%6.1f MB at least, %7.1f GB/s)   (b) statement + upload %9.1f ms   (b)/(a) %7.0f"
          % (name, t_d, nbytes / 1e6, nbytes / t_d / 1e6, t_h, t_h / t_d))
print("P_2 dofmap on the device: old mesh %.3f ms, refined mesh %.3f ms" % (t_map, t_map2))
print("(a) and (b) give the same bits: %s" % ("yes" if all(same) else "NO %s" % same))
