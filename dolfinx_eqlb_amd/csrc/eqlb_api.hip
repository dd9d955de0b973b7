// Host side of the C ABI (include/eqlb.h): device residency of mesh / patch SoA, binning of
// patches by size, kernel launches.  Mirrors the driver se::reconstruction<T>
// (cpp/dolfinx_eqlb/se/reconstruction.hpp:337-407) with the per-call setup hoisted into the
// handle.  There is NO CPU fallback: without a HIP device every compute entry point fails.
#include "eqlb_internal.h"
#include "eqlb_host_util.h"
#include "eqlb_topology_check.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <future>
#include <memory>
#include <mutex>
#include <thread>

namespace
{
thread_local std::string g_error;

} // namespace
namespace eqlb
{
// error message + code for the other translation units of the C ABI (eqlb_halo_rccl.hip)
int set_error(int code, const char* fmt, ...)
{
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_error = buf;
  return code;
}
} // namespace eqlb
namespace
{

void free_boundary(eqlb_se* h)
{
  dfree(h->facet_type);
  dfree(h->node_ws);
  dfree(h->node_group);
  dfree(h->node_wslevel);
  h->ws_levels = 1;
  dfree(h->rest_cells);
  h->nrest_cells = 0;
  dfree(h->bvals);
  dfree(h->node_slot);
  dfree(h->node_patch);
  dfree(h->slot_cell);
  dfree(h->slot_info);
  dfree(h->pn);
  dfree(h->pflag);
  dfree(h->slots); // re-zeroed on the next call (node_mask may have changed)
  dfree(h->l_off);
  dfree(h->l_slot_cell);
  dfree(h->l_slot_info);
  dfree(h->l_pflag);
  dfree(h->l_cells);
  dfree(h->l_ws);
  dfree(h->l_nodes);
  dfree(h->l_wsym_off);
  dfree(h->l_wsym_ws);
  dfree(h->l_rest_cells);
  h->l_nrest_cells = 0;
  h->l_stress = false;
  h->l_npatch = h->l_nslots = h->l_ncells = 0;
  h->l_maxcells = 0;
  dfree(h->t_tiles);
  dfree(h->t_tile_cells);
  dfree(h->t_facet_owner);
  dfree(h->t_slot_cell);
  dfree(h->t_slot_info);
  dfree(h->t_pn);
  dfree(h->t_pflag);
  h->ntiles = 0;
  h->t_mixed = false;
  std::fill(h->t_blocks, h->t_blocks + EQLB_TB_COUNT, int64_t(0));
  h->boundary_set = false;
}
// Grouped boundary patches of the stress path (se/reconstruction.hpp:170-234, se/Patch.cpp:60-104,
// 762-784; RT_2 only): a node whose two boundary facets carry flux BCs on both stress rows
// (base/BoundaryData.cpp:611-631) and that has two cells is grouped with the adjacent internal patch.
// The reference treats the groups one after the other in node order and lets the weak-symmetry step of a
// group see what the EARLIER groups added to the global stress on the cells of its internal patch
// (se/solve_patch_weaksym.hpp:100-131 reads the global vector).  On the device all row-wise sweeps come first
// and every (cell, vertex) contribution keeps its own slot row, so "what has been added so far" is a sum of
// slot rows: own row + rows of the vertices that are two-cell members of the own group + rows of the vertices
// that belong to an EARLIER group (group ids are handed out in the reference's discovery order; the patch
// builder marks those vertices).  The symmetry step of an earlier group has modified the rows of its internal
// patch, so overlapping groups are ordered: level of a group = 1 + the highest level among the earlier groups
// that own a vertex of one of its internal patch's cells; the weak-symmetry kernel runs level by level.
// ws: 0 normal, 1 two-cell member, 2 internal patch; level [nnodes]: level of the node's group (0 elsewhere).
int find_stress_groups(const eqlb::DeviceMesh& m, const int8_t* facet_type, const uint8_t* node_mask,
                       std::vector<int8_t>& ws, std::vector<int32_t>& group, std::vector<int8_t>& level,
                       int& nlevels, bool& any)
{
  const int32_t nn = m.nnodes;
  ws.assign(nn, 0);
  group.assign(nn, -1);
  any = false;
  std::vector<int8_t> cnt(nn, 0);
  for (int r = 0; r < 2; ++r)
    for (int32_t f = 0; f < m.nfacets; ++f)
      if (facet_type[(size_t)r * m.nfacets + f] == EQLB_FACET_ESSNT_DUAL)
      {
        ++cnt[m.h_facet_nodes[2 * (size_t)f]];
        ++cnt[m.h_facet_nodes[2 * (size_t)f + 1]];
      }
  int32_t ngroups = 0;
  for (int32_t node = 0; node < nn; ++node)
  {
    if (node_mask && !node_mask[node])
      continue;
    if (cnt[node] != 4 || group[node] >= 0 || m.h_node_ncells[node] != 2)
      continue;
    int32_t inner = -1;
    for (int32_t q = m.h_node_facets_off[node]; q < m.h_node_facets_off[node + 1] && inner < 0; ++q)
    {
      const int32_t f = m.h_node_facets[q];
      if (facet_type[f] == EQLB_FACET_INTERNAL)
        inner = (m.h_facet_nodes[2 * (size_t)f] == node) ? m.h_facet_nodes[2 * (size_t)f + 1]
                                                         : m.h_facet_nodes[2 * (size_t)f];
    }
    if (inner < 0)
      continue;
    std::vector<int32_t> members{inner};
    for (int32_t q = m.h_node_cells_off[inner]; q < m.h_node_cells_off[inner + 1]; ++q)
      for (int v = 0; v < 3; ++v)
      {
        const int32_t pnt = m.h_cell_nodes[3 * (size_t)m.h_node_cells[q] + v];
        if (cnt[pnt] == 4 && m.h_node_ncells[pnt] == 2
            && std::find(members.begin(), members.end(), pnt) == members.end())
          members.push_back(pnt);
      }
    if (members.size() < 2)
      continue;
    for (int32_t nd : members)
    {
      if (group[nd] >= 0 || (node_mask && !node_mask[nd]))
        return fail(EQLB_ERR_UNSUPPORTED,
                    "Incompatible mesh! To many patches with 2 cells on neumann boundary.");
      group[nd] = ngroups;
      ws[nd] = (nd == inner) ? 2 : 1;
    }
    ++ngroups;
    any = true;
  }
  // levels of overlapping groups (ascending group id = the reference's order)
  level.assign(nn, 0);
  nlevels = 1;
  if (any)
  {
    std::vector<int32_t> inner_of(ngroups, -1);
    for (int32_t node = 0; node < nn; ++node)
      if (ws[node] == 2)
        inner_of[group[node]] = node;
    std::vector<int> glevel(ngroups, 0);
    for (int32_t g = 0; g < ngroups; ++g)
    {
      const int32_t node = inner_of[g];
      int lv = 0;
      for (int32_t q = m.h_node_cells_off[node]; q < m.h_node_cells_off[node + 1]; ++q)
        for (int v = 0; v < 3; ++v)
        {
          const int32_t nd = m.h_cell_nodes[3 * (size_t)m.h_node_cells[q] + v];
          if (group[nd] >= 0 && group[nd] < g)
            lv = std::max(lv, glevel[group[nd]] + 1);
        }
      glevel[g] = lv;
      nlevels = std::max(nlevels, lv + 1);
    }
    if (nlevels > eqlb::WS_MAX_LEVELS)
      return fail(EQLB_ERR_UNSUPPORTED, "more than %d levels of overlapping groups of boundary patches",
                  eqlb::WS_MAX_LEVELS);
    for (int32_t node = 0; node < nn; ++node)
      if (group[node] >= 0)
        level[node] = (int8_t)glevel[group[node]];
  }
  return EQLB_OK;
}

} // namespace

extern "C" {


const char* eqlb_last_error(void) { return g_error.c_str(); }

int eqlb_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess)
    return 0;
  return n;
}

int eqlb_mesh_create(int32_t nnodes, int32_t ncells, int32_t nfacets, const double* x,
                     const int32_t* cell_nodes, const int32_t* cell_facets,
                     const int32_t* facet_nodes, const int32_t* facet_cells_offsets,
                     const int32_t* facet_cells, const int32_t* node_cells_offsets,
                     const int32_t* node_cells, const int32_t* node_facets_offsets,
                     const int32_t* node_facets, const uint8_t* facet_perm, eqlb_mesh_t** mesh)
try
{
  if (!mesh || nnodes <= 0 || ncells <= 0 || nfacets <= 0 || !x || !cell_nodes || !cell_facets
      || !facet_nodes || !facet_cells_offsets || !facet_cells || !node_cells_offsets || !node_cells
      || !node_facets_offsets || !node_facets || !facet_perm)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_mesh_create: null or empty input");
  if (eqlb_device_count() < 1)
    return fail(EQLB_ERR_DEVICE, "eqlb_mesh_create: no HIP device available");
  // The kernels index with these tables unchecked: a bad entry would fault on the device, so the
  // connectivities are validated here (O(size) on the host, once per mesh).
  {
    auto csr_ok = [](const int32_t* off, int32_t n, const int32_t* val, int32_t bound) {
      if (off[0] != 0)
        return false;
      for (int32_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i])
          return false;
      for (int32_t q = 0; q < off[n]; ++q)
        if (val[q] < 0 || val[q] >= bound)
          return false;
      return true;
    };
    bool ok = true;
    for (size_t i = 0; i < (size_t)ncells * 3 && ok; ++i)
      ok = cell_nodes[i] >= 0 && cell_nodes[i] < nnodes && cell_facets[i] >= 0 && cell_facets[i] < nfacets
           && facet_perm[i] <= 1;
    for (size_t i = 0; i < (size_t)nfacets * 2 && ok; ++i)
      ok = facet_nodes[i] >= 0 && facet_nodes[i] < nnodes;
    ok = ok && csr_ok(facet_cells_offsets, nfacets, facet_cells, ncells)
         && csr_ok(node_cells_offsets, nnodes, node_cells, ncells)
         && csr_ok(node_facets_offsets, nnodes, node_facets, nfacets);
    for (int32_t f = 0; f < nfacets && ok; ++f)
    {
      const int32_t nc = facet_cells_offsets[f + 1] - facet_cells_offsets[f];
      ok = (nc == 1 || nc == 2);
    }
    if (!ok)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_mesh_create: inconsistent connectivity tables");
  }
  eqlb_mesh* m = new eqlb_mesh();
  eqlb::DeviceMesh& d = m->m;
  d.nnodes = nnodes;
  d.ncells = ncells;
  d.nfacets = nfacets;
  d.h_node_ncells.resize(nnodes);
  d.h_node_nfcts.resize(nnodes);
  for (int32_t i = 0; i < nnodes; ++i)
  {
    d.h_node_ncells[i] = node_cells_offsets[i + 1] - node_cells_offsets[i];
    d.h_node_nfcts[i] = node_facets_offsets[i + 1] - node_facets_offsets[i];
    d.ncells_max = std::max(d.ncells_max, d.h_node_ncells[i]);
  }
  // One-cell facets per node: with the two counts above they tell whether the patch builder can walk the node (one
  // closed ring or one open fan, eqlb_topology_check.h).  Nothing is refused here: the local mesh of a rank
  // legitimately holds nodes it does not own at which two fans meet; eqlb_se_set_boundary refuses them when they are
  // to be equilibrated.
  d.h_node_nbnd.resize(nnodes);
  eqlb::count_node_boundary_facets(nnodes, node_facets_offsets, node_facets, facet_cells_offsets, d.h_node_nbnd.data());
  d.h_facet_cells_off.assign(facet_cells_offsets, facet_cells_offsets + (size_t)nfacets + 1);
  d.h_x.assign(x, x + (size_t)nnodes * 3);
  d.h_cell_nodes.assign(cell_nodes, cell_nodes + (size_t)ncells * 3);
  d.h_facet_nodes.assign(facet_nodes, facet_nodes + (size_t)nfacets * 2);
  d.h_node_facets_off.assign(node_facets_offsets, node_facets_offsets + (size_t)nnodes + 1);
  d.h_node_facets.assign(node_facets, node_facets + (size_t)node_facets_offsets[nnodes]);
  d.h_node_cells_off.assign(node_cells_offsets, node_cells_offsets + (size_t)nnodes + 1);
  d.h_node_cells.assign(node_cells, node_cells + (size_t)node_cells_offsets[nnodes]);
  int st = 0;
  st |= upload(&d.x, x, (size_t)nnodes * 3);
  st |= upload(&d.cell_nodes, cell_nodes, (size_t)ncells * 3);
  st |= upload(&d.cell_facets, cell_facets, (size_t)ncells * 3);
  st |= upload(&d.facet_nodes, facet_nodes, (size_t)nfacets * 2);
  st |= upload(&d.facet_cells_off, facet_cells_offsets, (size_t)nfacets + 1);
  st |= upload(&d.facet_cells, facet_cells, (size_t)facet_cells_offsets[nfacets]);
  st |= upload(&d.node_cells_off, node_cells_offsets, (size_t)nnodes + 1);
  st |= upload(&d.node_facets_off, node_facets_offsets, (size_t)nnodes + 1);
  st |= upload(&d.node_facets, node_facets, (size_t)node_facets_offsets[nnodes]);
  st |= upload(&d.facet_perm, facet_perm, (size_t)ncells * 3);
  st |= upload<double>(&d.cellJ, nullptr, (size_t)ncells * 4);
  if (st)
  {
    eqlb_mesh_destroy(m);
    return EQLB_ERR_DEVICE;
  }
  eqlb::launch_cell_geometry(ncells, d.x, d.cell_nodes, d.cellJ, nullptr);
  eqlb::device_tiling_prepare(); // code object of the tile builder loaded here, not inside the first set_boundary
  if (hipDeviceSynchronize() != hipSuccess)
  {
    eqlb_mesh_destroy(m);
    return fail(EQLB_ERR_DEVICE, "eqlb_mesh_create: geometry kernel failed");
  }
  *mesh = m;
  return EQLB_OK;
}
EQLB_CATCH_ALL

void eqlb_mesh_destroy(eqlb_mesh_t* m)
{
  if (!m)
    return;
  eqlb::DeviceMesh& d = m->m;
  dfree(d.x);
  dfree(d.cellJ);
  dfree(d.cell_nodes);
  dfree(d.cell_facets);
  dfree(d.facet_nodes);
  dfree(d.facet_cells_off);
  dfree(d.facet_cells);
  dfree(d.node_cells_off);
  dfree(d.node_facets_off);
  dfree(d.node_facets);
  dfree(d.node_cells);
  dfree(d.facet_perm);
  delete m;
}

int32_t eqlb_mesh_max_patch_cells(const eqlb_mesh_t* mesh) { return mesh ? mesh->m.ncells_max : 0; }

int eqlb_se_create(eqlb_mesh_t* mesh, int32_t k, int32_t degree_dg, int32_t nrhs,
                   int32_t reconstruct_stress, int32_t estimate_korn, eqlb_se_t** handle)
try
{
  if (!mesh || !handle || nrhs < 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "Equilibration: Input sizes does not match");
  if (k < 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "Degree must be at least 1");
  // se/reconstruction.hpp:363-373
  if (degree_dg > k - 1 || degree_dg < 0)
    return fail(EQLB_ERR_INVALID_ARGUMENT,
                "Equilibration: Wrong polynomial degree of the projected RHS");
  if (reconstruct_stress)
  {
    // se/reconstruction.hpp:376-388
    if (nrhs < 2)
      return fail(EQLB_ERR_INVALID_ARGUMENT,
                  "Stress equilibration: Specify all rows of stress tensor");
    if (k < 2)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "Stress equilibration: RT_k with k>1 required!");
  }
  (void)estimate_korn;
  std::vector<double> tab;
  if (eqlb::fill_tables_host(k, degree_dg, tab) != 0 || k > 4)
    return fail(EQLB_ERR_UNSUPPORTED, "RT_%d with DG_%d data%s is not in this build", k, degree_dg,
                reconstruct_stress ? " (stress)" : "");
  eqlb_se* h = new eqlb_se();
  h->mesh = mesh;
  h->k = k;
  h->deg = degree_dg;
  h->nrhs = nrhs;
  h->stress = reconstruct_stress ? 1 : 0;
  // default result path: tiled launch where it is the fastest (measured)
  h->scatter = EQLB_SCATTER_AUTO;
  // (k = 4, three interior unknowns per cell: register solver as well since round 3 - 0.38 ms against 14.9 ms of
  // the dense LDS Cholesky at 250 000 triangles; the EV patch problems at k = 4 stay on the dense solver)
  h->nrt = k * (k + 2);
  h->nd = (degree_dg + 1) * (degree_dg + 2) / 2;
  int st = upload(&h->tables, tab.data(), tab.size());
  st |= upload<int32_t>(&h->status, nullptr, 1);
  if (st)
  {
    eqlb_se_destroy(h);
    return EQLB_ERR_DEVICE;
  }
  (void)hipMemset(h->status, 0, sizeof(int32_t));
  *handle = h;
  return EQLB_OK;
}
EQLB_CATCH_ALL

void eqlb_se_destroy(eqlb_se_t* h)
{
  if (!h)
    return;
  free_boundary(h);
  dfree(h->tables);
  dfree(h->slots);
  dfree(h->status);
  dfree(h->d_flux_dg);
  dfree(h->d_rhs_dg);
  dfree(h->d_flux_hdiv);
  dfree(h->d_cks);
  dfree(h->d_korn);
  if (h->ev)
  {
    for (int i = 0; i < eqlb_se::EV_RING * eqlb_se::EV_PER_SET; ++i)
      if (h->ev[i])
        (void)hipEventDestroy(h->ev[i]);
    delete[] h->ev;
  }
  if (h->ev_fork)
    (void)hipEventDestroy(h->ev_fork);
  if (h->ev_join)
    (void)hipEventDestroy(h->ev_join);
  if (h->side_stream)
    (void)hipStreamDestroy(h->side_stream);
  delete h;
}

int eqlb_se_set_option(eqlb_se_t* h, const char* key, int32_t value)
{
  if (!h || !key)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_set_option: null argument");
  if (!strcmp(key, "solver"))
  {
#ifdef EQLB_EXP_SOLVER9 // timing-only variant without the solve (wrong results): experiment builds only
    const bool exp9 = value == 9;
#else
    const bool exp9 = false;
#endif
    if (value != EQLB_SOLVER_LDS_CHOLESKY && value != EQLB_SOLVER_SHUFFLE && !exp9)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "unknown solver %d", value);
    h->solver = value;
  }
  else if (!strcmp(key, "scatter"))
  {
    if (value != EQLB_SCATTER_SLOTS && value != EQLB_SCATTER_ATOMIC && value != EQLB_SCATTER_TILED
        && value != EQLB_SCATTER_AUTO)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "unknown scatter mode %d", value);
    h->scatter = value;
  }
  else if (!strcmp(key, "fused"))
    h->fused = value;
  else if (!strcmp(key, "timing"))
  {
    h->timing = value;
    h->ev_calls = 0;
  }
  else if (!strcmp(key, "accumulate"))
  {
    if (value != 0 && value != 1)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "accumulate must be 0 or 1");
    h->accumulate = value;
  }
  else if (!strcmp(key, "multi_rhs"))
  {
    if (value != 0 && value != 1)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "multi_rhs must be 0 or 1");
    h->multi_rhs = value;
  }
  else if (!strcmp(key, "large_patches"))
  {
    // takes effect at the next eqlb_se_set_boundary
    if (value != 0 && value != 1)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "large_patches must be 0 or 1");
    h->large_patches = value;
  }
  else if (!strcmp(key, "large_patches_stress"))
  {
    // takes effect at the next eqlb_se_set_boundary, on a handle with "large_patches" = 1
    if (value != 0 && value != 1)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "large_patches_stress must be 0 or 1");
    h->large_patches_stress = value;
  }
  else if (!strcmp(key, "tile_first"))
  {
    if (value < 0)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "tile_first must not be negative");
    h->tile_first = value;
  }
  else if (!strcmp(key, "tile_count"))
    h->tile_count = value;
  else if (!strcmp(key, "tile_cells"))
  {
    if (value < 0)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "tile_cells must not be negative");
    h->tile_cells_user = value;
  }
  else
    return fail(EQLB_ERR_INVALID_ARGUMENT, "unknown option '%s'", key);
  return EQLB_OK;
}

int eqlb_se_set_boundary(eqlb_se_t* h, const int8_t* facet_type, const double* boundary_values,
                         const uint8_t* node_mask)
try
{
  if (!h || !facet_type)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_set_boundary: null argument");
  SetupTimer tm;
  const eqlb::DeviceMesh& m = h->mesh->m;
  for (size_t i = 0; i < (size_t)h->nrhs * m.nfacets; ++i)
    if (facet_type[i] < EQLB_FACET_INTERNAL || facet_type[i] > EQLB_FACET_ESSNT_DUAL)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_set_boundary: facet type %d out of range", (int)facet_type[i]);
  bool inhomogeneous = false;
  if (boundary_values)
  {
    const size_t nb = (size_t)h->nrhs * m.ncells * h->nrt;
    for (size_t i = 0; i < nb && !inhomogeneous; ++i)
      inhomogeneous = (boundary_values[i] != 0.0);
  }
  // (into a local: the handle is not touched before the last check that can refuse the table with the old boundary
  // data still in place; the sweep reads h->stress_flux_bcs)
  bool stress_flux_bcs = false;
  if (h->stress)
    for (size_t i = 0; i < (size_t)2 * m.nfacets && !stress_flux_bcs; ++i)
      stress_flux_bcs = (facet_type[i] == EQLB_FACET_ESSNT_DUAL);
  // RT_2 stress: the fused tiled launch (k_se_stress_tiled) reads DG_1 data; DG_0 data take the route of stress flux
  // BCs - rows into the slots by the patch kernels of the handle's degree, then the weak-symmetry kernel of that route
  // (launch_se_weaksym with no_flux_bcs = false; it reads no DG data, nor do the Korn kernels)
  const bool stress_fused_ok = h->k == 2 && h->deg == 1 && !stress_flux_bcs;
  // OrientedPatch::set_max_patch_size (se/Patch.cpp:337-404): every local node is checked
  for (int32_t i = 0; i < m.nnodes; ++i)
  {
    if (node_mask && !node_mask[i])
      continue; // the reference loops the owned nodes only (size_local)
    if (m.h_node_ncells[i] == 1)
      return fail(EQLB_ERR_PATCH_TOO_SMALL, "Patch around node %d has only 1 cells.", i);
    if (m.h_node_ncells[i] < 1)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "node %d belongs to no cell", i);
  }
  // What the patch builder cannot walk (eqlb_topology_check.h), refused before the old tables are freed: a refused
  // call leaves the handle as it was.  Facets both of whose nodes are masked out are not looked at.
  {
    const eqlb::TopoFinding tf = eqlb::check_boundary_topology(
        m.nnodes, m.nfacets, h->nrhs, m.h_node_ncells.data(), m.h_node_nfcts.data(), m.h_node_nbnd.data(),
        m.h_facet_nodes.data(), m.h_facet_cells_off.data(), facet_type, node_mask);
    if (tf.verdict == eqlb::TOPO_NODE_NOT_WALKABLE)
      return fail(EQLB_ERR_UNSUPPORTED,
                  "Patch around node %d (%d cells, %d facets, %d of them boundary facets) is neither one closed ring nor "
                  "one open fan of cells: a vertex where the boundary touches itself cannot be equilibrated",
                  tf.index, m.h_node_ncells[tf.index], m.h_node_nfcts[tf.index], m.h_node_nbnd[tf.index]);
    if (tf.verdict == eqlb::TOPO_BOUNDARY_FACET_UNTYPED)
      return fail(EQLB_ERR_INVALID_ARGUMENT,
                  "eqlb_se_set_boundary: boundary facet %d (nodes %d, %d) has type 0 on right-hand side %d: every "
                  "facet with one cell at an equilibrated node needs a boundary condition",
                  tf.index, m.h_facet_nodes[2 * (size_t)tf.index], m.h_facet_nodes[2 * (size_t)tf.index + 1], tf.row);
    if (tf.verdict == eqlb::TOPO_INTERIOR_FACET_TYPED)
      return fail(EQLB_ERR_INVALID_ARGUMENT,
                  "eqlb_se_set_boundary: facet %d (nodes %d, %d) lies between two cells and has type %d on right-hand "
                  "side %d: only facets with one cell carry boundary conditions",
                  tf.index, m.h_facet_nodes[2 * (size_t)tf.index], m.h_facet_nodes[2 * (size_t)tf.index + 1],
                  (int)facet_type[(size_t)tf.row * m.nfacets + tf.index], tf.row);
  }
  tm.lap("checks");
  free_boundary(h);
  h->stress_flux_bcs = stress_flux_bcs;
  tm.lap("free old tables");

  // bins by lanes per patch: P = smallest of {4,8,16,32,64} >= number of patch facets
  std::vector<int64_t> node_slot(m.nnodes, -1), node_patch(m.nnodes, -1);
  int64_t count[eqlb::MAX_BINS] = {0, 0, 0, 0, 0};
  std::vector<int8_t> node_bin(m.nnodes, -1);
  std::vector<int32_t> large_nodes; // patches of more than 63 cells or more than 64 facets
  for (int32_t i = 0; i < m.nnodes; ++i)
  {
    if (node_mask && !node_mask[i])
      continue;
    const int nf = m.h_node_nfcts[i];
    int b = 0;
    while (b < eqlb::MAX_BINS && eqlb::BIN_P[b] < nf)
      ++b;
    if (b == eqlb::MAX_BINS || m.h_node_ncells[i] > 63)
    {
      if (!h->large_patches)
        return fail(EQLB_ERR_PATCH_TOO_LARGE, "Patch around node %d has %d cells (limit 63)", i,
                    m.h_node_ncells[i]);
      // option "large_patches": the patch goes to the multi-wave kernel (a CSR-style SoA of its own, below); its node
      // stays out of the bins and is, for the tiles, a node that another path equilibrates
      if (h->stress && !h->large_patches_stress)
        return fail(EQLB_ERR_PATCH_TOO_LARGE,
                    "Patch around node %d has %d cells: the stress equilibration (weak symmetry, Korn constants) is "
                    "limited to 63 cells per patch, \"large_patches\" covers flux equilibration only",
                    i, m.h_node_ncells[i]);
      if (h->mode == 1 && h->k >= 4)
        return fail(EQLB_ERR_PATCH_TOO_LARGE,
                    "Patch around node %d has %d cells: the constrained minimisation at RT_4 is limited to 63 cells per "
                    "patch, \"large_patches\" covers it for RT_1 ... RT_3",
                    i, m.h_node_ncells[i]);
      large_nodes.push_back(i);
      continue;
    }
    node_bin[i] = (int8_t)b;
    ++count[b];
  }
  int64_t slot_off = 0, patch_off = 0;
  for (int b = 0; b < eqlb::MAX_BINS; ++b)
  {
    h->bins[b].P = eqlb::BIN_P[b];
    h->bins[b].npatch = count[b];
    h->bins[b].slot_offset = slot_off;
    h->bins[b].patch_offset = patch_off;
    slot_off += count[b] * eqlb::BIN_P[b];
    patch_off += count[b];
    count[b] = 0;
  }
  h->nslots = slot_off;
  h->npatch_total = patch_off;
  // fused stress launch (RT_2, no flux BCs on the stress rows): it takes the FULL patches of the bins 0, 1 -
  // interior, as many cells as lanes -, listed first in their bin; the generic kernels take the patches behind them
  const bool full_first = h->stress && stress_fused_ok && h->mode == 0;
  auto is_full = [&](int32_t i) {
    const int b = node_bin[i];
    return full_first && b >= 0 && b < 2 && m.h_node_ncells[i] == m.h_node_nfcts[i]
           && m.h_node_ncells[i] == eqlb::BIN_P[b];
  };
  for (int pass = 0; pass < 2; ++pass)
  {
    for (int32_t i = 0; i < m.nnodes; ++i)
    {
      const int b = node_bin[i];
      if (b < 0 || is_full(i) != (pass == 0))
        continue;
      node_patch[i] = h->bins[b].patch_offset + count[b];
      node_slot[i] = h->bins[b].slot_offset + count[b] * eqlb::BIN_P[b];
      ++count[b];
    }
    if (pass == 0)
      for (int b = 0; b < eqlb::MAX_BINS; ++b)
        h->bins[b].nfull = count[b];
  }

  tm.lap("binning");
  int st = 0;
  st |= upload(&h->facet_type, facet_type, (size_t)h->nrhs * m.nfacets);
  if (inhomogeneous)
    st |= upload(&h->bvals, boundary_values, (size_t)h->nrhs * m.ncells * h->nrt);
  st |= upload(&h->node_slot, node_slot.data(), (size_t)m.nnodes);
  st |= upload(&h->node_patch, node_patch.data(), (size_t)m.nnodes);
  st |= upload<int32_t>(&h->slot_cell, nullptr, (size_t)h->nslots);
  st |= upload<uint32_t>(&h->slot_info, nullptr, (size_t)h->nslots);
  st |= upload<uint8_t>(&h->pn, nullptr, (size_t)h->npatch_total);
  st |= upload<uint8_t>(&h->pflag, nullptr, (size_t)h->npatch_total * h->nrhs);
  if (st)
    return EQLB_ERR_DEVICE;
  HIP_TRY(hipMemset(h->slot_cell, 0xff, sizeof(int32_t) * std::max<int64_t>(h->nslots, 1)));
  HIP_TRY(hipMemset(h->slot_info, 0, sizeof(uint32_t) * std::max<int64_t>(h->nslots, 1)));

  eqlb::BuildArgs a{};
  a.nnodes = m.nnodes;
  a.nfacets = m.nfacets;
  a.nrhs = h->nrhs;
  a.cell_nodes = m.cell_nodes;
  a.cell_facets = m.cell_facets;
  a.facet_nodes = m.facet_nodes;
  a.facet_cells_off = m.facet_cells_off;
  a.facet_cells = m.facet_cells;
  a.node_cells_off = m.node_cells_off;
  a.node_facets_off = m.node_facets_off;
  a.node_facets = m.node_facets;
  a.facet_perm = m.facet_perm;
  a.facet_type = h->facet_type;
  if (h->stress && h->k == 2 && h->stress_flux_bcs)
  {
    std::vector<int8_t> ws, lvl;
    std::vector<int32_t> grp;
    bool any = false;
    h->ws_levels = 1;
    const int stg = find_stress_groups(m, facet_type, node_mask, ws, grp, lvl, h->ws_levels, any);
    if (stg)
      return stg;
    // a large patch inside a group (its two-cell members never are large): the weak-symmetry kernel of the large
    // patches does not read the rows of other patches
    for (int32_t nd : large_nodes)
      if (any && ws[nd] != 0)
        return fail(EQLB_ERR_UNSUPPORTED,
                    "Patch around node %d has %d cells and is the internal patch of group %d of boundary patches with "
                    "tractions on both stress rows: groups are limited to 63 cells per patch (\"large_patches_stress\")",
                    nd, m.h_node_ncells[nd], grp[nd]);
    if (any)
    {
      if (upload(&h->node_ws, ws.data(), ws.size()) || upload(&h->node_group, grp.data(), grp.size())
          || upload(&h->node_wslevel, lvl.data(), lvl.size()))
        return EQLB_ERR_DEVICE;
      a.node_ws = h->node_ws;
      a.node_group = h->node_group;
      a.node_wslevel = h->node_wslevel;
    }
  }
  a.node_slot = h->node_slot;
  a.node_patch = h->node_patch;
  a.npatch_total = h->npatch_total;
  a.slot_cell = h->slot_cell;
  a.slot_info = h->slot_info;
  a.pn = h->pn;
  a.pflag = h->pflag;
  a.stride = 0;
  eqlb::launch_build_patches(a, nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  tm.lap("plain SoA: upload + builder");
  if (!large_nodes.empty())
  {
    // large patches: lane slots in CSR form (l_off), the same descriptor bits, flags per right-hand side; the cell
    // count of a patch is the difference of its offsets
    const int64_t nl = (int64_t)large_nodes.size();
    std::vector<int64_t> lslot(m.nnodes, -1), lpatch(m.nnodes, -1);
    std::vector<int32_t> off(nl + 1, 0);
    std::vector<uint8_t> is_large(m.nnodes, 0);
    int64_t acc = 0;
    for (int64_t p = 0; p < nl; ++p)
    {
      const int32_t nd = large_nodes[p];
      lslot[nd] = acc;
      lpatch[nd] = p;
      is_large[nd] = 1;
      off[p] = (int32_t)acc;
      acc += m.h_node_ncells[nd];
      h->l_maxcells = std::max(h->l_maxcells, m.h_node_ncells[nd]);
      if (acc > 0x7fffff00)
        return fail(EQLB_ERR_UNSUPPORTED, "large-patch SoA exceeds 2^31 lane slots");
    }
    off[nl] = (int32_t)acc;
    std::vector<int32_t> lc;
    for (int32_t c = 0; c < m.ncells; ++c)
      for (int j = 0; j < 3; ++j)
        if (is_large[m.h_cell_nodes[3 * (size_t)c + j]])
        {
          lc.push_back(c);
          break;
        }
    int64_t *d_lslot = nullptr, *d_lpatch = nullptr;
    int stl = 0;
    stl |= upload(&h->l_off, off.data(), off.size());
    stl |= upload<int32_t>(&h->l_slot_cell, nullptr, (size_t)acc);
    stl |= upload<uint32_t>(&h->l_slot_info, nullptr, (size_t)acc);
    stl |= upload<uint8_t>(&h->l_pflag, nullptr, (size_t)nl * h->nrhs);
    stl |= upload(&h->l_cells, lc.data(), lc.size());
    stl |= upload<double>(&h->l_ws, nullptr, eqlb::large_patch_ws_doubles(h->k, acc, nl));
    stl |= upload(&h->l_nodes, large_nodes.data(), large_nodes.size());
    if (h->stress)
    {
      // work space of the weak-symmetry kernel: per patch, quadratic in its cells (the Schur matrix)
      std::vector<int64_t> woff(nl + 1, 0);
      for (int64_t p = 0; p < nl; ++p)
        woff[p + 1] = woff[p] + (int64_t)eqlb::large_patch_weaksym_ws_doubles(h->k, m.h_node_ncells[large_nodes[p]]);
      stl |= upload(&h->l_wsym_off, woff.data(), (size_t)nl);
      stl |= upload<double>(&h->l_wsym_ws, nullptr, (size_t)woff[nl]);
    }
    stl |= upload(&d_lslot, lslot.data(), lslot.size());
    stl |= upload(&d_lpatch, lpatch.data(), lpatch.size());
    hipError_t e = hipSuccess;
    if (!stl)
    {
      eqlb::BuildArgs al = a;
      al.node_ws = nullptr;
      al.node_slot = d_lslot;
      al.node_patch = d_lpatch;
      al.npatch_total = nl;
      al.slot_cell = h->l_slot_cell;
      al.slot_info = h->l_slot_info;
      al.pn = nullptr;
      al.pflag = h->l_pflag;
      al.large = 1;
      eqlb::launch_build_patches(al, nullptr);
      e = hipGetLastError();
      if (e == hipSuccess)
        e = hipDeviceSynchronize();
    }
    dfree(d_lslot);
    dfree(d_lpatch);
    if (stl)
      return EQLB_ERR_DEVICE;
    if (e != hipSuccess)
      return fail(EQLB_ERR_DEVICE, "large-patch builder: %s", hipGetErrorString(e));
    h->l_npatch = nl;
    h->l_nslots = acc;
    h->l_ncells = (int64_t)lc.size();
    h->l_stress = h->large_patches_stress != 0;
    tm.lap("large-patch SoA");
  }
  h->t_stress = h->stress && stress_fused_ok && h->mode == 0;
  if (h->t_stress || (!h->stress && h->k <= 3))
  {
    // fused stress launch: its own tile size, patches of up to 8 facets (bins 0, 1)
    h->t_mixed = false;
    if (h->t_stress)
    {
      // Patches of the bins 0, 1 that are not full (interior with fewer cells than lanes, boundary): on the crossed
      // benchmark meshes the boundary patches only (0.4 %) - the tiles list the full patches and the others go with
      // the rest (generic kernels on a side stream next to the fused kernel); on unstructured meshes most patches -
      // the tiles list every patch of the two bins and the kernel carries both instances of the body.
      // EQLB_STRESS_MIXED_TILES=0/1 forces the choice.
      int64_t nlisted = 0, nnotfull = 0;
      for (int32_t i = 0; i < m.nnodes; ++i)
      {
        const int8_t b = node_bin[i];
        if (b < 0 || b >= 2)
          continue;
        ++nlisted;
        if (!(m.h_node_ncells[i] == m.h_node_nfcts[i] && m.h_node_ncells[i] == eqlb::BIN_P[b]))
          ++nnotfull;
      }
      h->t_mixed = nnotfull * 20 > nlisted;
      if (const char* env = getenv("EQLB_STRESS_MIXED_TILES"))
        h->t_mixed = env[0] != '0';
    }
    const int stt = h->t_stress ? eqlb::build_tiles(h, node_bin, a, eqlb::stress_tile_cells(), 2, !h->t_mixed)
                                : eqlb::build_tiles(h, node_bin, a);
    if (stt)
      return stt;
    if (h->mode == 1)
    {
      const int64_t ne = (int64_t)h->ntiles * h->tile_tc * 3;
      if (upload<int32_t>(&h->t_facet_owner, nullptr, (size_t)std::max<int64_t>(ne, 1)))
        return EQLB_ERR_DEVICE;
      eqlb::launch_tile_facet_owner(m, ne, h->t_tile_cells, h->t_facet_owner, nullptr);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipDeviceSynchronize());
    }
  }
  if (h->t_stress && h->l_npatch > 0)
  {
    // fused stress launch: the rows of the rest and of the large patches go through the slot buffer together; one
    // compact reduction over the cells that either of them touches
    std::vector<uint8_t> touched(m.nnodes, 0);
    for (int32_t i = 0; i < m.nnodes; ++i)
      touched[i] = (!node_mask || node_mask[i]) && (node_bin[i] < 0 || node_bin[i] >= 2 || (!h->t_mixed && !is_full(i)));
    std::vector<int32_t> rc;
    for (int32_t c = 0; c < m.ncells; ++c)
      for (int j = 0; j < 3; ++j)
        if (touched[m.h_cell_nodes[3 * (size_t)c + j]])
        {
          rc.push_back(c);
          break;
        }
    h->l_nrest_cells = (int64_t)rc.size();
    if (upload(&h->l_rest_cells, rc.data(), rc.size()))
      return EQLB_ERR_DEVICE;
  }
  tm.lap("tiles (total)");
  h->boundary_set = true;
  return EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_se_kornconst(eqlb_se_t* h, double* cells_kornconst, int32_t memspace, void* stream_)
try
{
  if (!h || !cells_kornconst)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "Equilibration: Input sizes does not match");
  if (!h->boundary_set)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_kornconst: boundary data not set");
  if (h->l_npatch > 0 && !h->l_stress)
    return fail(EQLB_ERR_PATCH_TOO_LARGE,
                "eqlb_se_kornconst: the Korn constants are limited to 63 cells per patch, \"large_patches\" covers flux "
                "equilibration only");
  const eqlb::DeviceMesh& m = h->mesh->m;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!h->d_cks && upload<double>(&h->d_cks, nullptr, (size_t)m.nnodes))
    return EQLB_ERR_DEVICE;
  double* d_korn = cells_kornconst;
  if (memspace == EQLB_MEM_HOST)
  {
    if (!h->d_korn && upload<double>(&h->d_korn, nullptr, (size_t)m.ncells))
      return EQLB_ERR_DEVICE;
    HIP_TRY(hipMemcpyAsync(h->d_korn, cells_kornconst, sizeof(double) * m.ncells, hipMemcpyHostToDevice, stream));
    d_korn = h->d_korn;
  }
  eqlb::launch_korn(m, h->node_slot, h->node_patch, h->slot_cell, h->slot_info, h->pn, h->pflag,
                    h->d_cks, d_korn, stream, h->l_npatch, h->l_nodes, h->l_off, h->l_slot_cell, h->l_slot_info,
                    h->l_pflag);
  HIP_TRY(hipGetLastError());
  if (memspace == EQLB_MEM_HOST)
  {
    HIP_TRY(hipMemcpyAsync(cells_kornconst, d_korn, sizeof(double) * m.ncells, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
  }
  return EQLB_OK;
}
EQLB_CATCH_ALL

int64_t eqlb_se_num_patches(const eqlb_se_t* h) { return h ? h->npatch_total : 0; }

int eqlb_se_tiling_info(const eqlb_se_t* h, int64_t* ntiles, int64_t* cells_per_tile,
                        int64_t* npatch_instances, int64_t* nlane_slots)
{
  if (!h || !h->boundary_set)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_tiling_info: set the boundary first");
  if (ntiles)
    *ntiles = h->ntiles;
  if (cells_per_tile)
    *cells_per_tile = h->tile_tc;
  if (npatch_instances)
    *npatch_instances = h->t_npatch;
  if (nlane_slots)
    *nlane_slots = h->t_nslots;
  return EQLB_OK;
}

int eqlb_se_tiling_blocks(const eqlb_se_t* h, int64_t* out, int32_t n)
{
  if (!h || !h->boundary_set)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_tiling_blocks: set the boundary first");
  if (n < 0 || (n > 0 && !out))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_tiling_blocks: invalid argument");
  for (int32_t i = 0; i < std::min<int32_t>(n, EQLB_TB_COUNT); ++i)
    out[i] = h->ntiles > 0 ? h->t_blocks[i] : 0;
  return EQLB_OK;
}

int eqlb_se_large_patch_info(const eqlb_se_t* h, int64_t* npatches, int32_t* max_cells)
{
  if (!h || !h->boundary_set)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_large_patch_info: set the boundary first");
  if (npatches)
    *npatches = h->l_npatch;
  if (max_cells)
    *max_cells = h->l_maxcells;
  return EQLB_OK;
}

int eqlb_se_set_priority_cells(eqlb_se_t* h, const int32_t* cells, int32_t n)
try
{
  if (!h || n < 0 || (n > 0 && !cells))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_set_priority_cells: invalid argument");
  h->prio_cells.assign(cells, cells + n);
  return EQLB_OK;
}
EQLB_CATCH_ALL

int32_t eqlb_se_num_priority_tiles(const eqlb_se_t* h) { return (h && h->boundary_set) ? h->t_nprio : 0; }

int eqlb_se_export_patches(eqlb_se_t* h, int32_t stride, int32_t* ncells, int32_t* cells,
                           int32_t* fcts, int8_t* fcts_local, int8_t* inodes_local,
                           int8_t* reversed)
try
{
  if (!h || !ncells || !cells || !fcts || !fcts_local || !inodes_local || !reversed)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_export_patches: null argument");
  if (!h->boundary_set)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_export_patches: set the boundary first");
  const eqlb::DeviceMesh& m = h->mesh->m;
  if (stride < m.ncells_max + 2)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_export_patches: stride too small");
  const size_t nn = (size_t)m.nnodes;
  int32_t *d_n = nullptr, *d_c = nullptr, *d_f = nullptr;
  int8_t *d_fl = nullptr, *d_il = nullptr, *d_rv = nullptr;
  int st = 0;
  st |= upload<int32_t>(&d_n, nullptr, nn);
  st |= upload<int32_t>(&d_c, nullptr, nn * stride);
  st |= upload<int32_t>(&d_f, nullptr, nn * stride);
  st |= upload<int8_t>(&d_fl, nullptr, nn * stride * 2);
  st |= upload<int8_t>(&d_il, nullptr, nn * stride);
  st |= upload<int8_t>(&d_rv, nullptr, nn * stride * 2);
  if (!st)
  {
    eqlb::BuildArgs a{};
    a.nnodes = m.nnodes;
    a.nfacets = m.nfacets;
    a.nrhs = h->nrhs;
    a.cell_nodes = m.cell_nodes;
    a.cell_facets = m.cell_facets;
    a.facet_nodes = m.facet_nodes;
    a.facet_cells_off = m.facet_cells_off;
    a.facet_cells = m.facet_cells;
    a.node_cells_off = m.node_cells_off;
    a.node_facets_off = m.node_facets_off;
    a.node_facets = m.node_facets;
    a.facet_perm = m.facet_perm;
    a.facet_type = h->facet_type;
    a.node_slot = nullptr;
    a.node_patch = nullptr;
    a.npatch_total = 0;
    a.large = h->large_patches; // fans of more than 63 cells as well (the stride holds them)
    a.stride = stride;
    a.ex_ncells = d_n;
    a.ex_cells = d_c;
    a.ex_fcts = d_f;
    a.ex_fl = d_fl;
    a.ex_il = d_il;
    a.ex_rev = d_rv;
    eqlb::launch_build_patches(a, nullptr);
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess)
      e = hipMemcpy(ncells, d_n, nn * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess)
      e = hipMemcpy(cells, d_c, nn * stride * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess)
      e = hipMemcpy(fcts, d_f, nn * stride * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess)
      e = hipMemcpy(fcts_local, d_fl, nn * stride * 2, hipMemcpyDeviceToHost);
    if (e == hipSuccess)
      e = hipMemcpy(inodes_local, d_il, nn * stride, hipMemcpyDeviceToHost);
    if (e == hipSuccess)
      e = hipMemcpy(reversed, d_rv, nn * stride * 2, hipMemcpyDeviceToHost);
    if (e != hipSuccess)
      st = fail(EQLB_ERR_DEVICE, "eqlb_se_export_patches: %s", hipGetErrorString(e));
  }
  dfree(d_n);
  dfree(d_c);
  dfree(d_f);
  dfree(d_fl);
  dfree(d_il);
  dfree(d_rv);
  return st ? EQLB_ERR_DEVICE : EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_project_dg(eqlb_mesh_t* mesh, int32_t degree, int32_t bs, int32_t nrhs, int32_t nq,
                    const double* qpoints, const double* qweights, const double* qvalues,
                    double* out, int32_t memspace, void* stream_)
try
{
  if (!mesh || !qpoints || !qweights || !qvalues || !out || bs < 1 || nrhs < 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "Local solver: Input sizes does not match");
  std::vector<double> Pm;
  const int st = eqlb::projection_matrix_host(degree, nq, qpoints, qweights, Pm);
  if (st)
    return fail(st, "eqlb_project_dg: unsupported degree %d or number of points %d", degree, nq);
  const int nd = (degree + 1) * (degree + 2) / 2;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const int64_t ncells = (int64_t)mesh->m.ncells * nrhs; // the RHS are stacked cell blocks
  const size_t n_in = (size_t)ncells * nq * bs, n_out = (size_t)ncells * nd * bs;
  double *d_P = nullptr, *d_in = nullptr, *d_out = nullptr;
  if (upload(&d_P, Pm.data(), Pm.size()))
    return EQLB_ERR_DEVICE;
  int rc = EQLB_OK;
  if (memspace == EQLB_MEM_HOST)
  {
    if (upload(&d_in, qvalues, n_in) || upload<double>(&d_out, nullptr, n_out))
      rc = EQLB_ERR_DEVICE;
  }
  else
  {
    d_in = const_cast<double*>(qvalues);
    d_out = out;
  }
  if (!rc)
  {
    eqlb::launch_project_dg(ncells, nd, nq, bs, d_P, d_in, d_out, stream);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && memspace == EQLB_MEM_HOST)
      e = hipMemcpy(out, d_out, n_out * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess)
      e = hipStreamSynchronize(stream); // d_P is freed below
    if (e != hipSuccess)
      rc = fail(EQLB_ERR_DEVICE, "eqlb_project_dg: %s", hipGetErrorString(e));
  }
  dfree(d_P);
  if (memspace == EQLB_MEM_HOST)
  {
    dfree(d_in);
    dfree(d_out);
  }
  return rc;
}
EQLB_CATCH_ALL

int eqlb_get_reference_table(int32_t k, int32_t degree_dg, const char* name, double* out,
                             int32_t capacity)
{
  std::vector<double> tab;
  if (!name || !out || eqlb::fill_tables_host(k, degree_dg, tab) != 0)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_get_reference_table: unknown table");
  const int nrt = k * (k + 2), nd = (degree_dg + 1) * (degree_dg + 2) / 2, nq = k * (k + 1) / 2;
  // layout of the table buffer (fill_tables_host): S | F | H | D | ...; the three rows of H are padded
  // to an even number of doubles there (Sizes::HROW) and returned without the padding
  const size_t hrow = (size_t)nd * nq, hrow_pad = hrow + (hrow & 1);
  const size_t nS = (size_t)3 * nrt * nrt, nF = (size_t)9 * nd * k, nH = 3 * hrow, nHp = 3 * hrow_pad,
               nD = (size_t)6 * nd * nq;
  size_t off = 0, len = 0;
  if (!strcmp(name, "S"))
  {
    off = 0;
    len = nS;
  }
  else if (!strcmp(name, "F"))
  {
    off = nS;
    len = nF;
  }
  else if (!strcmp(name, "H"))
  {
    if ((size_t)capacity < nH)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_get_reference_table: capacity too small");
    for (int n = 0; n < 3; ++n)
      std::copy(tab.begin() + nS + nF + n * hrow_pad, tab.begin() + nS + nF + n * hrow_pad + hrow,
                out + n * hrow);
    return (int)nH;
  }
  else if (!strcmp(name, "D"))
  {
    off = nS + nF + nHp;
    len = nD;
  }
  else
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_get_reference_table: unknown table '%s'", name);
  if ((size_t)capacity < len)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_get_reference_table: capacity too small");
  std::copy(tab.begin() + off, tab.begin() + off + len, out);
  return (int)len;
}

// degree of the projected data of an estimator call: 0 ... k - 1 (the pairs the tables exist for)
static int check_degree_dg(const char* who, int32_t k, int32_t degree_dg)
{
  if (degree_dg < 0 || degree_dg > k - 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: Wrong polynomial degree of the projected RHS (degree_dg = %d, k = %d)",
                who, (int)degree_dg, (int)k);
  return EQLB_OK;
}

static int estimate_impl(eqlb_mesh_t* mesh, int32_t k, int32_t degree_dg, int32_t nrhs, const double* flux_hdiv,
                         const double* flux_dg, const double* rhs_dg, double* cell_div2,
                         double* cell_sig2, double* facet_jump, int32_t memspace, void* stream_,
                         double alpha, double beta)
{
  if (!mesh || !flux_hdiv || !flux_dg || !rhs_dg || nrhs < 1 || k < 1 || k > 4)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_estimate: invalid argument");
  if (check_degree_dg("eqlb_se_estimate", k, degree_dg))
    return EQLB_ERR_INVALID_ARGUMENT;
  const eqlb::DeviceMesh& m = mesh->m;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const int nrt = k * (k + 2), nd = (degree_dg + 1) * (degree_dg + 2) / 2;
  const size_t n_x = (size_t)nrhs * m.ncells * nrt, n_g = (size_t)nrhs * m.ncells * nd * 2,
               n_f = (size_t)nrhs * m.ncells * nd;
  const size_t n_c = (size_t)nrhs * m.ncells, n_e = (size_t)nrhs * m.nfacets;
  if (memspace == EQLB_MEM_DEVICE)
  {
    const int st = eqlb::launch_estimate(m, k, degree_dg, nrhs, flux_hdiv, flux_dg, rhs_dg, cell_div2, cell_sig2,
                                         facet_jump, alpha, beta, stream);
    return st ? fail(st, "eqlb_se_estimate: kernel launch failed") : EQLB_OK;
  }
  if (memspace != EQLB_MEM_HOST)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_estimate: unknown memory space");
  double *d_x = nullptr, *d_g = nullptr, *d_f = nullptr, *d_d = nullptr, *d_s = nullptr, *d_j = nullptr;
  int st = upload(&d_x, flux_hdiv, n_x) | upload(&d_g, flux_dg, n_g) | upload(&d_f, rhs_dg, n_f);
  if (cell_div2)
    st |= upload<double>(&d_d, nullptr, n_c);
  if (cell_sig2)
    st |= upload<double>(&d_s, nullptr, n_c);
  if (facet_jump)
    st |= upload<double>(&d_j, nullptr, n_e);
  int rc = st ? EQLB_ERR_DEVICE : eqlb::launch_estimate(m, k, degree_dg, nrhs, d_x, d_g, d_f, d_d, d_s, d_j, alpha, beta,
                                                        stream);
  hipError_t e = hipSuccess;
  if (!rc && cell_div2)
    e = hipMemcpy(cell_div2, d_d, n_c * sizeof(double), hipMemcpyDeviceToHost);
  if (!rc && e == hipSuccess && cell_sig2)
    e = hipMemcpy(cell_sig2, d_s, n_c * sizeof(double), hipMemcpyDeviceToHost);
  if (!rc && e == hipSuccess && facet_jump)
    e = hipMemcpy(facet_jump, d_j, n_e * sizeof(double), hipMemcpyDeviceToHost);
  dfree(d_x);
  dfree(d_g);
  dfree(d_f);
  dfree(d_d);
  dfree(d_s);
  dfree(d_j);
  if (rc || e != hipSuccess)
    return fail(EQLB_ERR_DEVICE, "eqlb_se_estimate: device error");
  return EQLB_OK;
}

int eqlb_se_estimate(eqlb_mesh_t* mesh, int32_t k, int32_t nrhs, const double* flux_hdiv,
                     const double* flux_dg, const double* rhs_dg, double* cell_div2,
                     double* cell_sig2, double* facet_jump, int32_t memspace, void* stream)
{
  return estimate_impl(mesh, k, k - 1, nrhs, flux_hdiv, flux_dg, rhs_dg, cell_div2, cell_sig2, facet_jump,
                       memspace, stream, 0.0, 1.0);
}

int eqlb_se_estimate_dg(eqlb_mesh_t* mesh, int32_t k, int32_t degree_dg, int32_t nrhs, const double* flux_hdiv,
                        const double* flux_dg, const double* rhs_dg, double* cell_div2, double* cell_sig2,
                        double* facet_jump, int32_t memspace, void* stream)
{
  return estimate_impl(mesh, k, degree_dg, nrhs, flux_hdiv, flux_dg, rhs_dg, cell_div2, cell_sig2, facet_jump,
                       memspace, stream, 0.0, 1.0);
}

int eqlb_ev_estimate(eqlb_mesh_t* mesh, int32_t k, int32_t nrhs, const double* flux_broken,
                     const double* flux_dg, const double* rhs_dg, double* cell_div2,
                     double* cell_sig2, double* facet_jump, int32_t memspace, void* stream)
{
  return estimate_impl(mesh, k, k - 1, nrhs, flux_broken, flux_dg, rhs_dg, cell_div2, cell_sig2, facet_jump,
                       memspace, stream, -1.0, 0.0);
}

int eqlb_ev_estimate_dg(eqlb_mesh_t* mesh, int32_t k, int32_t degree_dg, int32_t nrhs, const double* flux_broken,
                        const double* flux_dg, const double* rhs_dg, double* cell_div2, double* cell_sig2,
                        double* facet_jump, int32_t memspace, void* stream)
{
  return estimate_impl(mesh, k, degree_dg, nrhs, flux_broken, flux_dg, rhs_dg, cell_div2, cell_sig2, facet_jump,
                       memspace, stream, -1.0, 0.0);
}

// Host arrays of a call staged on the device for its duration (inputs copied in, outputs copied back).
namespace
{
struct Staging
{
  std::vector<double*> bufs;
  struct Out
  {
    double *host, *dev;
    size_t n;
  };
  std::vector<Out> outs;
  bool bad = false;
  const double* in(const double* host, size_t n)
  {
    if (!host)
      return nullptr;
    double* d = nullptr;
    if (upload(&d, host, n))
      bad = true;
    bufs.push_back(d);
    return d;
  }
  double* out(double* host, size_t n)
  {
    if (!host)
      return nullptr;
    double* d = nullptr;
    if (upload<double>(&d, nullptr, n))
      bad = true;
    bufs.push_back(d);
    outs.push_back({host, d, n});
    return d;
  }
  bool fetch()
  {
    for (const Out& o : outs)
      if (hipMemcpy(o.host, o.dev, o.n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
        return false;
    return true;
  }
  ~Staging()
  {
    for (double* b : bufs)
      if (b)
        (void)hipFree(b);
  }
};
} // namespace

int eqlb_se_estimate_stress(eqlb_mesh_t* mesh, int32_t k, const double* flux_hdiv, const double* korn,
                            double pi_1, double* cell_energy, double* cell_wsym, double* node_asym,
                            int32_t memspace, void* stream_)
{
  if (!mesh || !flux_hdiv || k < 1 || k > 4 || !(pi_1 > -1.0))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_estimate_stress: invalid argument");
  if (memspace != EQLB_MEM_DEVICE && memspace != EQLB_MEM_HOST)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_estimate_stress: unknown memory space");
  eqlb::DeviceMesh& m = mesh->m;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (node_asym)
  {
    std::lock_guard<std::mutex> g(mesh->tiling_mutex); // (the mesh-level lock: first use from several threads)
    if (!m.node_cells && upload(&m.node_cells, m.h_node_cells.data(), m.h_node_cells.size()))
      return fail(EQLB_ERR_DEVICE, "eqlb_se_estimate_stress: device allocation failed");
  }
  const size_t nx = (size_t)m.ncells * k * (k + 2);
  int rc;
  if (memspace == EQLB_MEM_DEVICE)
    rc = eqlb::launch_estimate_stress(m, m.node_cells, k, flux_hdiv, flux_hdiv + nx, korn, pi_1, cell_energy,
                                      cell_wsym, node_asym, stream);
  else
  {
    Staging s;
    const double* d_x = s.in(flux_hdiv, 2 * nx);
    const double* d_k = s.in(korn, m.ncells);
    double* d_e = s.out(cell_energy, m.ncells);
    double* d_w = s.out(cell_wsym, m.ncells);
    double* d_a = s.out(node_asym, m.nnodes);
    if (s.bad)
      return fail(EQLB_ERR_DEVICE, "eqlb_se_estimate_stress: device allocation failed");
    rc = eqlb::launch_estimate_stress(m, m.node_cells, k, d_x, d_x + nx, d_k, pi_1, d_e, d_w, d_a, stream);
    if (!rc && !s.fetch())
      rc = EQLB_ERR_DEVICE;
  }
  return rc ? fail(rc, "eqlb_se_estimate_stress: device error") : EQLB_OK;
}

int eqlb_oscillation(eqlb_mesh_t* mesh, int32_t k, int32_t nrhs, const double* flux, const double* flux_dg,
                     int32_t nq, const double* qpoints, const double* qweights, const double* fvalues,
                     const double* korn, double* out, int32_t memspace, void* stream)
{
  return eqlb_oscillation_dg(mesh, k, k - 1, nrhs, flux, flux_dg, nq, qpoints, qweights, fvalues, korn, out,
                             memspace, stream);
}

int eqlb_oscillation_dg(eqlb_mesh_t* mesh, int32_t k, int32_t degree_dg, int32_t nrhs, const double* flux,
                        const double* flux_dg, int32_t nq, const double* qpoints, const double* qweights,
                        const double* fvalues, const double* korn, double* out, int32_t memspace, void* stream_)
{
  if (!mesh || !flux || !qpoints || !qweights || !fvalues || !out || nrhs < 1 || k < 1 || k > 4 || nq < 1
      || nq > 128)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_oscillation: invalid argument");
  if (memspace != EQLB_MEM_DEVICE && memspace != EQLB_MEM_HOST)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_oscillation: unknown memory space");
  if (check_degree_dg("eqlb_oscillation", k, degree_dg))
    return EQLB_ERR_INVALID_ARGUMENT;
  const eqlb::DeviceMesh& m = mesh->m;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const size_t nx = (size_t)nrhs * m.ncells * k * (k + 2),
               ng = (size_t)nrhs * m.ncells * (degree_dg + 1) * (degree_dg + 2);
  int rc;
  if (memspace == EQLB_MEM_DEVICE)
    rc = eqlb::launch_oscillation(m, k, degree_dg, nrhs, flux, flux_dg, nq, qpoints, qweights, fvalues, korn, out,
                                  stream);
  else
  {
    Staging s;
    const double* d_x = s.in(flux, nx);
    const double* d_g = s.in(flux_dg, ng);
    const double* d_f = s.in(fvalues, (size_t)nrhs * m.ncells * nq);
    const double* d_k = s.in(korn, m.ncells);
    double* d_o = s.out(out, (size_t)nrhs * m.ncells);
    if (s.bad)
      return fail(EQLB_ERR_DEVICE, "eqlb_oscillation: device allocation failed");
    rc = eqlb::launch_oscillation(m, k, degree_dg, nrhs, d_x, d_g, nq, qpoints, qweights, d_f, d_k, d_o, stream);
    if (!rc && !s.fetch())
      rc = EQLB_ERR_DEVICE;
  }
  return rc ? fail(rc, "eqlb_oscillation: device error") : EQLB_OK;
}

int eqlb_boundary_residual(eqlb_mesh_t* mesh, int32_t k, int32_t degree_dg, int32_t nrhs, const double* flux,
                           const double* flux_dg, int32_t nfacets_bc, const int32_t* facets,
                           const double* boundary_values, double* out, int32_t memspace, void* stream_)
{
  if (!mesh || !flux || nrhs < 1 || k < 1 || k > 4 || nfacets_bc < 0 || (nfacets_bc > 0 && (!facets || !out)))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_boundary_residual: invalid argument");
  if (memspace != EQLB_MEM_DEVICE && memspace != EQLB_MEM_HOST)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_boundary_residual: unknown memory space");
  if (check_degree_dg("eqlb_boundary_residual", k, degree_dg))
    return EQLB_ERR_INVALID_ARGUMENT;
  const eqlb::DeviceMesh& m = mesh->m;
  if (memspace == EQLB_MEM_HOST)
    for (int32_t i = 0; i < nfacets_bc; ++i)
      if (facets[i] < 0 || facets[i] >= m.nfacets)
        return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_boundary_residual: facets[%d] = %d is no facet of the mesh",
                    (int)i, (int)facets[i]);
  if (nfacets_bc == 0)
    return EQLB_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const size_t nx = (size_t)nrhs * m.ncells * k * (k + 2),
               ng = (size_t)nrhs * m.ncells * (degree_dg + 1) * (degree_dg + 2);
  int rc;
  if (memspace == EQLB_MEM_DEVICE)
    rc = eqlb::launch_boundary_residual(m, k, degree_dg, nrhs, flux, flux_dg, nfacets_bc, facets, boundary_values,
                                        out, stream);
  else
  {
    Staging s;
    const double* d_x = s.in(flux, nx);
    const double* d_g = s.in(flux_dg, ng);
    const double* d_b = s.in(boundary_values, nx);
    double* d_o = s.out(out, (size_t)nrhs * nfacets_bc);
    int32_t* d_l = nullptr;
    if (upload(&d_l, facets, (size_t)nfacets_bc))
      s.bad = true;
    rc = s.bad ? EQLB_ERR_DEVICE
               : eqlb::launch_boundary_residual(m, k, degree_dg, nrhs, d_x, d_g, nfacets_bc, d_l, d_b, d_o, stream);
    if (!rc && !s.fetch())
      rc = EQLB_ERR_DEVICE;
    dfree(d_l);
  }
  return rc ? fail(rc, "eqlb_boundary_residual: device error") : EQLB_OK;
}

int eqlb_halo_pack(int32_t nrhs, int32_t nlist, int32_t nrt, int64_t ncells, const int64_t* cells,
                   double* x, double* buf, int32_t clear, void* stream)
{
  if (nrhs < 0 || nlist < 0 || nrt < 1 || (nlist > 0 && (!cells || !x || !buf)))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_halo_pack: invalid argument");
  eqlb::launch_halo_pack(nrhs, nlist, nrt, ncells, cells, x, buf, clear, reinterpret_cast<hipStream_t>(stream));
  return (hipGetLastError() == hipSuccess) ? EQLB_OK : fail(EQLB_ERR_DEVICE, "eqlb_halo_pack: launch failed");
}

int eqlb_halo_unpack_add(int32_t nrhs, int32_t nlist, int32_t nrt, int64_t ncells, const int64_t* cells,
                         double* x, const double* buf, void* stream)
{
  if (nrhs < 0 || nlist < 0 || nrt < 1 || (nlist > 0 && (!cells || !x || !buf)))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_halo_unpack_add: invalid argument");
  eqlb::launch_halo_unpack_add(nrhs, nlist, nrt, ncells, cells, x, buf, reinterpret_cast<hipStream_t>(stream));
  return (hipGetLastError() == hipSuccess) ? EQLB_OK
                                           : fail(EQLB_ERR_DEVICE, "eqlb_halo_unpack_add: launch failed");
}

// ---- constrained-minimisation (EV) equilibrator ---------------------------------------------------
int eqlb_ev_create(eqlb_mesh_t* mesh, int32_t k, int32_t nrhs, eqlb_ev_t** handle)
{
  return eqlb_ev_create_dg(mesh, k, k - 1, nrhs, handle);
}

int eqlb_ev_create_dg(eqlb_mesh_t* mesh, int32_t k, int32_t degree_dg, int32_t nrhs, eqlb_ev_t** handle)
try
{
  if (!handle)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_ev_create: null argument");
  eqlb_se* se = nullptr;
  const int st = eqlb_se_create(mesh, k, degree_dg, nrhs, 0, 0, &se);
  if (st)
    return st;
  se->mode = 1;
  se->ev_ndofs = (int64_t)mesh->m.nfacets * k + (int64_t)mesh->m.ncells * (k * k - k);
  eqlb_ev* h = new eqlb_ev();
  h->se = se;
  *handle = h;
  return EQLB_OK;
}
EQLB_CATCH_ALL

void eqlb_ev_destroy(eqlb_ev_t* h)
{
  if (!h)
    return;
  if (h->se)
  {
    dfree(h->se->ev_cell_dofs);
    dfree(h->se->ev_basis);
    eqlb_se_destroy(h->se);
  }
  delete h;
}

int eqlb_ev_set_option(eqlb_ev_t* h, const char* key, int32_t value)
{
  if (!h || !key)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_ev_set_option: null argument");
  if (!strcmp(key, "output"))
  {
    if (value != 0 && value != 1)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "unknown output layout %d", value);
    h->se->ev_output = value;
    dfree(h->se->d_flux_hdiv); // staging size depends on the layout
    dfree(h->se->d_flux_dg);
    dfree(h->se->d_rhs_dg);
    return EQLB_OK;
  }
  if (!strcmp(key, "boundary_basis"))
  {
    if (value != 0 && value != 1)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "unknown boundary basis %d", value);
    h->se->ev_bv_hier = value;
    return EQLB_OK;
  }
  if (!strcmp(key, "timing") || !strcmp(key, "scatter") || !strcmp(key, "accumulate") || !strcmp(key, "tile_cells")
      || !strcmp(key, "multi_rhs") || !strcmp(key, "large_patches"))
    return eqlb_se_set_option(h->se, key, value);
  return fail(EQLB_ERR_INVALID_ARGUMENT, "unknown option '%s'", key);
}

int eqlb_ev_set_dofmap(eqlb_ev_t* h, const int32_t* cell_dofs, int64_t ndofs)
try
{
  if (!h)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_ev_set_dofmap: null argument");
  eqlb_se* se = h->se;
  const eqlb::DeviceMesh& m = se->mesh->m;
  dfree(se->ev_cell_dofs);
  dfree(se->d_flux_hdiv);
  dfree(se->d_flux_dg);
  dfree(se->d_rhs_dg);
  if (!cell_dofs)
  {
    se->ev_ndofs = (int64_t)m.nfacets * se->k + (int64_t)m.ncells * (se->k * se->k - se->k);
    return EQLB_OK;
  }
  const size_t n = (size_t)m.ncells * se->nrt;
  for (size_t i = 0; i < n; ++i)
    if (cell_dofs[i] < 0 || cell_dofs[i] >= ndofs)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_ev_set_dofmap: DOF %d out of range", cell_dofs[i]);
  if (upload(&se->ev_cell_dofs, cell_dofs, n))
    return EQLB_ERR_DEVICE;
  se->ev_ndofs = ndofs;
  return EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_ev_set_basis_transform(eqlb_ev_t* h, const double* C, const double* R)
{
  if (!h)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_ev_set_basis_transform: null argument");
  eqlb_se* se = h->se;
  dfree(se->ev_basis);
  se->ev_basis_has_R = false;
  if (!C)
    return EQLB_OK;
  const int nrt = se->nrt, k = se->k;
  // facet rows of C must not see anything but their own facet block (the other functions of the
  // hierarchic element have no normal trace there): the two cells of a facet would disagree otherwise
  for (int f = 0; f < 3; ++f)
    for (int j = 0; j < k; ++j)
      for (int c = 0; c < nrt; ++c)
        if ((c < f * k || c >= (f + 1) * k) && C[(f * k + j) * nrt + c] != 0.0)
          return fail(EQLB_ERR_INVALID_ARGUMENT,
                      "eqlb_ev_set_basis_transform: facet DOF %d of the target element depends on DOF %d outside its "
                      "facet", f * k + j, c);
  // [C | R | facet maps]: broken facet DOFs = (facet block of C)^-1 [R^-1] x target facet DOFs, for the boundary values
  std::vector<double> buf((size_t)nrt * nrt + k * k + 6 * k * k, 0.0);
  std::copy(C, C + (size_t)nrt * nrt, buf.begin());
  double* Rd = buf.data() + (size_t)nrt * nrt;
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < k; ++j)
      Rd[i * k + j] = R ? R[i * k + j] : (i == j ? 1.0 : 0.0);
  auto invert = [k](const double* A, double* Ai) -> bool { // Gauss-Jordan with partial pivoting, k <= 4
    double w[4][8];
    for (int i = 0; i < k; ++i)
      for (int j = 0; j < k; ++j)
      {
        w[i][j] = A[i * k + j];
        w[i][k + j] = (i == j) ? 1.0 : 0.0;
      }
    for (int c = 0; c < k; ++c)
    {
      int p = c;
      for (int r = c + 1; r < k; ++r)
        if (std::fabs(w[r][c]) > std::fabs(w[p][c]))
          p = r;
      if (w[p][c] == 0.0)
        return false;
      for (int j = 0; j < 2 * k; ++j)
        std::swap(w[c][j], w[p][j]);
      const double ip = 1.0 / w[c][c];
      for (int j = 0; j < 2 * k; ++j)
        w[c][j] *= ip;
      for (int r = 0; r < k; ++r)
        if (r != c)
        {
          const double f_ = w[r][c];
          for (int j = 0; j < 2 * k; ++j)
            w[r][j] -= f_ * w[c][j];
        }
    }
    for (int i = 0; i < k; ++i)
      for (int j = 0; j < k; ++j)
        Ai[i * k + j] = w[i][k + j];
    return true;
  };
  double Ri[16], Cf[16], Cfi[16];
  if (!invert(Rd, Ri))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_ev_set_basis_transform: R is singular");
  double* maps = Rd + k * k;
  for (int f = 0; f < 3; ++f)
  {
    for (int i = 0; i < k; ++i)
      for (int j = 0; j < k; ++j)
        Cf[i * k + j] = C[(f * k + i) * nrt + f * k + j];
    if (!invert(Cf, Cfi))
      return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_ev_set_basis_transform: facet block %d of C is singular", f);
    for (int i = 0; i < k; ++i)
      for (int j = 0; j < k; ++j)
      {
        maps[((f * 2 + 0) * k + i) * k + j] = Cfi[i * k + j];
        double a_ = 0.0;
        for (int q = 0; q < k; ++q)
          a_ += Cfi[i * k + q] * Ri[q * k + j];
        maps[((f * 2 + 1) * k + i) * k + j] = a_;
      }
  }
  if (upload(&se->ev_basis, buf.data(), buf.size()))
    return EQLB_ERR_DEVICE;
  se->ev_basis_has_R = R != nullptr;
  return EQLB_OK;
}

int64_t eqlb_ev_num_dofs(const eqlb_ev_t* h) { return h ? h->se->ev_ndofs : 0; }

int eqlb_ev_set_boundary(eqlb_ev_t* h, const int8_t* facet_type, const double* boundary_values,
                         const uint8_t* node_mask)
try
{
  if (!h)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_ev_set_boundary: null argument");
  eqlb_se* se = h->se;
  const int st = eqlb_se_set_boundary(se, facet_type, nullptr, node_mask);
  if (st)
    return st;
  const eqlb::DeviceMesh& m = se->mesh->m;
  bool inhomogeneous = false;
  const size_t nb = (size_t)se->nrhs * se->ev_ndofs;
  if (boundary_values)
    for (size_t i = 0; i < nb && !inhomogeneous; ++i)
      inhomogeneous = (boundary_values[i] != 0.0);
  if (inhomogeneous)
  {
    // conforming boundary DOFs -> the broken per-cell layout the patch kernel reads
    double* d_conf = nullptr;
    if (upload(&d_conf, boundary_values, nb)
        || upload<double>(&se->bvals, nullptr, (size_t)se->nrhs * m.ncells * se->nrt))
    {
      dfree(d_conf);
      return EQLB_ERR_DEVICE;
    }
    hipError_t e = hipMemset(se->bvals, 0, sizeof(double) * (size_t)se->nrhs * m.ncells * se->nrt);
    if (e == hipSuccess)
    {
      eqlb::launch_ev_boundary_to_broken(m, se->k, se->nrhs, se->ev_cell_dofs, se->ev_ndofs, d_conf, se->bvals,
                                         (se->ev_basis && !se->ev_bv_hier) ? se->ev_basis + se->nrt * se->nrt + se->k * se->k : nullptr, nullptr);
      e = hipDeviceSynchronize();
    }
    dfree(d_conf);
    if (e != hipSuccess)
      return fail(EQLB_ERR_DEVICE, "eqlb_ev_set_boundary: %s", hipGetErrorString(e));
  }
  return EQLB_OK;
}
EQLB_CATCH_ALL

int64_t eqlb_ev_num_patches(const eqlb_ev_t* h) { return h ? h->se->npatch_total : 0; }

int eqlb_ev_large_patch_info(const eqlb_ev_t* h, int64_t* npatches, int32_t* max_cells)
{
  if (!h)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_ev_large_patch_info: null handle");
  return eqlb_se_large_patch_info(h->se, npatches, max_cells);
}

int eqlb_ev_tiling_blocks(const eqlb_ev_t* h, int64_t* out, int32_t n)
{
  if (!h)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_ev_tiling_blocks: null handle");
  return eqlb_se_tiling_blocks(h->se, out, n);
}

} // extern "C"
