// The handle behind eqlb_mesh_t: owner of the device arrays of a mesh, of the host copies the planners read and of the
// tiling cache.  Host code only: for the units that dereference an eqlb_mesh; kernel files see eqlb::DeviceMesh alone.
#pragma once

#include "eqlb_boundary_plan.h"
#include "eqlb_host_util.h"

#include <map>
#include <mutex>

struct eqlb_mesh
{
  // the view the launchers take: the counts, and the pointers of the buffers below - null until publish(), so no
  // launcher may see it before
  eqlb::DeviceMesh m;
  eqlb::HostMesh host;
  eqlb::DevBuf<double> x, cellJ;
  eqlb::DevBuf<int32_t> cell_nodes, cell_facets, facet_nodes, facet_cells_off, facet_cells;
  eqlb::DevBuf<int32_t> node_cells_off, node_facets_off, node_facets;
  eqlb::DevBuf<int32_t> node_cells; // eqlb_mesh_create leaves it on the host: mesh_node_cells uploads it on first use
  eqlb::DevBuf<uint8_t> facet_perm;
  // the one place where the view learns of the buffers: the creators call it when every buffer is allocated
  void publish()
  {
    m.x = x, m.cellJ = cellJ, m.cell_nodes = cell_nodes, m.cell_facets = cell_facets, m.facet_nodes = facet_nodes;
    m.facet_cells_off = facet_cells_off, m.facet_cells = facet_cells, m.node_cells_off = node_cells_off;
    m.node_facets_off = node_facets_off, m.node_facets = node_facets, m.node_cells = node_cells;
    m.facet_perm = facet_perm;
  }
  std::mutex tiling_mutex; // the lock of the handle: the tiling cache and the first use of node_cells
  // cells in the order of the tile bisection (sorted by cell id inside every tile), per tile size: the tiling
  // depends on the mesh alone, so further handles on the mesh (SE + EV, a stress handle ...) and further
  // eqlb_se_set_boundary calls reuse it
  std::map<int, std::vector<int32_t>> tiling_order;
  // nodes of the cells of zero area (mesh_flat_nodes): found once per mesh, empty on a mesh without such a cell
  bool flat_known = false;
  std::vector<uint8_t> flat_nodes;
};

namespace eqlb
{
// node -> cell on the device, uploaded by the first caller.  Several host threads may come first at once: the table is
// copied under the lock of the handle (a copy from pageable memory has finished when it returns) and the view shows
// the pointer only afterwards
inline int mesh_node_cells(eqlb_mesh* mesh, const int32_t** out)
{
  std::lock_guard<std::mutex> g(mesh->tiling_mutex);
  if (!mesh->m.node_cells)
  {
    DevBuf<int32_t> fresh;
    EQLB_TRY(fresh.upload(mesh->host.node_cells.data(), mesh->host.node_cells.size()));
    mesh->node_cells = std::move(fresh);
    mesh->m.node_cells = mesh->node_cells;
  }
  *out = mesh->m.node_cells;
  return EQLB_OK;
}

// The vertices of the cells whose det J is zero to rounding or not finite (launch_flat_cell_nodes): *out is [nnodes], 1
// at such a vertex, or nullptr on a mesh without such a cell.  The element matrices of a flat cell are inf and NaN, so no
// patch that holds one can be equilibrated; the handles leave those patches out and report them (eqlb_se_set_boundary).
// One kernel over the cells and a copy of four bytes at the first call on a mesh, the answer is kept
inline int mesh_flat_nodes(eqlb_mesh* mesh, const uint8_t** out)
{
  std::lock_guard<std::mutex> g(mesh->tiling_mutex);
  if (!mesh->flat_known)
  {
    const DeviceMesh& m = mesh->m;
    DevBuf<uint8_t> flags;
    DevBuf<int32_t> count;
    if (flags.alloc((size_t)m.nnodes) || count.alloc(1))
      return EQLB_ERR_DEVICE;
    HIP_TRY(hipMemset(flags, 0, (size_t)m.nnodes));
    HIP_TRY(hipMemset(count, 0, sizeof(int32_t)));
    launch_flat_cell_nodes(m.ncells, m.cellJ, m.cell_nodes, flags, count, nullptr);
    HIP_TRY(hipGetLastError());
    int32_t n = 0;
    HIP_TRY(hipMemcpy(&n, count, sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<uint8_t> nodes;
    if (n > 0)
    {
      nodes.resize((size_t)m.nnodes);
      HIP_TRY(hipMemcpy(nodes.data(), flags, nodes.size(), hipMemcpyDeviceToHost));
    }
    mesh->flat_nodes = std::move(nodes);
    mesh->flat_known = true;
  }
  *out = mesh->flat_nodes.empty() ? nullptr : mesh->flat_nodes.data();
  return EQLB_OK;
}
} // namespace eqlb
