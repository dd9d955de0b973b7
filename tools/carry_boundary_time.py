"""Time of carrying the boundary conditions of an RT_2 handle across one refinement step at 1M triangles (crossed
500 x 500, the mesh and the marked list of tools/refine_time.py: eqlb_mark_doerfler on lognormal(0, 2) indicators at
theta = 0.5, about 2 % of the cells), median of 5 after one warm-up run each, with a device synchronisation on either
side.  Flux conditions on the sides x = 0 and y = 0 with a linear field, Dirichlet elsewhere.  Two routes to the handle
on the refined mesh:
  (a) carry:  eqlb_se_carry_boundary - types gathered on the device, eqlb_se_set_boundary without values, the table
              carried from table to table by one kernel
  (b) host:   the numpy statement (carry_facet_types, prolong_flux_bc) on host arrays, the dense table
              [1][ncells2 * 8] scattered from it, eqlb_se_set_boundary with that table (which uploads it); the
              download of the old table that precedes it is not counted
and, next to them, eqlb_se_set_boundary alone on the refined mesh (types of the statement, no values) - the host
planner both routes share - and the three device entries on their own.  The host side depends on the CPU."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from dolfinx_eqlb_amd import cpp
from dolfinx_eqlb_amd.mesh import carry_facet_types, create_unit_square, prolong_flux_bc
from synthetic import boundary_dofs_from_field, facet_types

REPEAT = 5
K = 2
NRT = K * (K + 2)


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


def w_lin(x, y):
    return 0.3 + 0.5 * x - 0.2 * y, -0.6 + 0.1 * x + 0.4 * y


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
pc, npf, pf = (t.cpu().numpy() for t in (r.parent_cell, r.node_parent_facet, r.parent_facet))
print("%d cells, %d marked -> %d cells, %d facets" % (n, int(nmarked.item()), n2, mesh2.nfacets))

ft = facet_types(mesh, lambda p: (p[:, 0] < 1e-9) | (p[:, 1] < 1e-9))
bv = boundary_dofs_from_field(mesh, K, ft[0], w_lin)[None]
old = cpp.SemiExplicitEquilibrator(dm, K, 1)
old.set_boundary(ft, boundary_values=bv)
fresh = cpp.SemiExplicitEquilibrator(r.dmesh, K, 1)
ft2 = carry_facet_types(ft, pf)
facets2 = np.nonzero(ft2[0] == 2)[0].astype(np.int32)
print("%d flux-BC facets -> %d" % (np.count_nonzero(ft[0] == 2), facets2.size))


def scatter(dofs):
    cells = mesh2.facet_cells[mesh2.facet_cells_offsets[facets2]]
    lf = np.argmax(mesh2.cell_facets[cells] == facets2[:, None], axis=1)
    table = np.zeros((1, n2 * NRT))
    for j in range(K):
        table[0, cells * NRT + lf * K + j] = dofs[:, j]
    return table


def route_carry():
    fresh.carry_boundary(old, r, stream=st)


def route_host():
    types2 = carry_facet_types(ft, pf)
    f2 = np.nonzero(types2[0] == 2)[0].astype(np.int32)
    fresh.set_boundary(types2, boundary_values=scatter(prolong_flux_bc(mesh, mesh2, pc, npf, K, bv[0], f2)))


def planner_alone():
    fresh.set_boundary(ft2)


d_ft, d_bv, d_f2 = torch.from_numpy(ft).to("cuda"), torch.from_numpy(bv).to("cuda"), torch.from_numpy(facets2).to("cuda")
d_bf = torch.from_numpy(np.nonzero(ft[0] > 0)[0].astype(np.int32)).to("cuda")
t_carry, t_host, t_plan = median_ms(route_carry), median_ms(route_host), median_ms(planner_alone)
route_carry()
table_a = fresh.get_boundary_values()
route_host()
same = np.array_equal(table_a, fresh.get_boundary_values()) and bool(np.abs(table_a).max() > 0)
t_types = median_ms(lambda: r.facet_types(d_ft, stream=st))
t_child = median_ms(lambda: r.child_facets(d_bf, stream=st))
t_vals = median_ms(lambda: r.prolong_flux_bc(K, d_bv, d_f2, stream=st))
print("(a) eqlb_se_carry_boundary            %9.1f ms" % t_carry)
print("(b) statement + set_boundary(table)   %9.1f ms   (b)/(a) %5.2f" % (t_host, t_host / t_carry))
print("    eqlb_se_set_boundary alone        %9.1f ms   (%.0f %% of (a))" % (t_plan, 100.0 * t_plan / t_carry))
print("device entries: facet types %.3f ms (%d facets), child facets %.3f ms (%d listed), flux-BC values %.3f ms (%d listed)"
      % (t_types, mesh2.nfacets, t_child, d_bf.numel(), t_vals, facets2.size))
print("(a) and (b) leave the same table: %s" % ("yes" if same else "NO"))
