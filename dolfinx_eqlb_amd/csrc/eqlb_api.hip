// Host side of the C ABI (include/eqlb.h): device residency of the mesh, the handles and their options, the
// entries around the sweep (Korn constants, patch export, projection, estimators).  Mirrors the driver
// se::reconstruction<T> (cpp/dolfinx_eqlb/se/reconstruction.hpp:337-407) with the per-call setup hoisted into the
// handle: eqlb_boundary_setup.hip builds the patch SoA, eqlb_sweep.hip runs the equilibration.  There is NO CPU
// fallback: without a HIP device every compute entry point fails.
#include "eqlb_handle.h"

#include <algorithm>
#include <cstdlib>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>

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
  std::unique_ptr<eqlb_mesh> m(new eqlb_mesh());
  eqlb::DeviceMesh& d = m->m;
  eqlb::HostMesh& hm = m->host;
  d.nnodes = nnodes;
  d.ncells = ncells;
  d.nfacets = nfacets;
  hm.node_ncells.resize(nnodes);
  hm.node_nfcts.resize(nnodes);
  for (int32_t i = 0; i < nnodes; ++i)
  {
    hm.node_ncells[i] = node_cells_offsets[i + 1] - node_cells_offsets[i];
    hm.node_nfcts[i] = node_facets_offsets[i + 1] - node_facets_offsets[i];
    d.ncells_max = std::max(d.ncells_max, hm.node_ncells[i]);
  }
  // One-cell facets per node: with the two counts above they tell whether the patch builder can walk the node (one
  // closed ring or one open fan, eqlb_topology_check.h).  Nothing is refused here: the local mesh of a rank
  // legitimately holds nodes it does not own at which two fans meet; eqlb_se_set_boundary refuses them when they are
  // to be equilibrated.
  hm.node_nbnd.resize(nnodes);
  eqlb::count_node_boundary_facets(nnodes, node_facets_offsets, node_facets, facet_cells_offsets, hm.node_nbnd.data());
  hm.facet_cells_off.assign(facet_cells_offsets, facet_cells_offsets + (size_t)nfacets + 1);
  hm.x.assign(x, x + (size_t)nnodes * 3);
  hm.cell_nodes.assign(cell_nodes, cell_nodes + (size_t)ncells * 3);
  hm.facet_nodes.assign(facet_nodes, facet_nodes + (size_t)nfacets * 2);
  hm.node_facets_off.assign(node_facets_offsets, node_facets_offsets + (size_t)nnodes + 1);
  hm.node_facets.assign(node_facets, node_facets + (size_t)node_facets_offsets[nnodes]);
  hm.node_cells_off.assign(node_cells_offsets, node_cells_offsets + (size_t)nnodes + 1);
  hm.node_cells.assign(node_cells, node_cells + (size_t)node_cells_offsets[nnodes]);
  int st = 0;
  st |= m->x.upload(x, (size_t)nnodes * 3);
  st |= m->cell_nodes.upload(cell_nodes, (size_t)ncells * 3);
  st |= m->cell_facets.upload(cell_facets, (size_t)ncells * 3);
  st |= m->facet_nodes.upload(facet_nodes, (size_t)nfacets * 2);
  st |= m->facet_cells_off.upload(facet_cells_offsets, (size_t)nfacets + 1);
  st |= m->facet_cells.upload(facet_cells, (size_t)facet_cells_offsets[nfacets]);
  st |= m->node_cells_off.upload(node_cells_offsets, (size_t)nnodes + 1);
  st |= m->node_facets_off.upload(node_facets_offsets, (size_t)nnodes + 1);
  st |= m->node_facets.upload(node_facets, (size_t)node_facets_offsets[nnodes]);
  st |= m->facet_perm.upload(facet_perm, (size_t)ncells * 3);
  st |= m->cellJ.alloc((size_t)ncells * 4);
  if (st)
    return EQLB_ERR_DEVICE;
  m->publish();
  eqlb::launch_cell_geometry(ncells, d.x, d.cell_nodes, d.cellJ, nullptr);
  eqlb::device_tiling_prepare(); // code object of the tile builder loaded here, not inside the first set_boundary
  if (hipDeviceSynchronize() != hipSuccess)
    return fail(EQLB_ERR_DEVICE, "eqlb_mesh_create: geometry kernel failed");
  *mesh = m.release();
  return EQLB_OK;
}
EQLB_CATCH_ALL

void eqlb_mesh_destroy(eqlb_mesh_t* m) { delete m; }

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
  std::unique_ptr<eqlb_se> h(new eqlb_se());
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
  if (h->tables.upload(tab.data(), tab.size()) || h->status.alloc(1))
    return EQLB_ERR_DEVICE;
  (void)hipMemset(h->status, 0, sizeof(int32_t));
  *handle = h.release();
  return EQLB_OK;
}
EQLB_CATCH_ALL

void eqlb_se_destroy(eqlb_se_t* h) { delete h; }

int eqlb_se_set_option(eqlb_se_t* h, const char* key, int32_t value)
{
  if (!h || !key)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_set_option: null argument");
  if (!strcmp(key, "solver"))
  {
    if (value != EQLB_SOLVER_LDS_CHOLESKY && value != EQLB_SOLVER_SHUFFLE)
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

int eqlb_se_kornconst(eqlb_se_t* h, double* cells_kornconst, int32_t memspace, void* stream_)
try
{
  if (!h || !cells_kornconst)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "Equilibration: Input sizes does not match");
  if (!h->bt.boundary_set)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_kornconst: boundary data not set");
  if (h->bt.l_npatch > 0 && !h->bt.l_stress)
    return fail(EQLB_ERR_PATCH_TOO_LARGE,
                "eqlb_se_kornconst: the Korn constants are limited to 63 cells per patch, \"large_patches\" covers flux "
                "equilibration only");
  const eqlb::DeviceMesh& m = h->mesh->m;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!h->d_cks && h->d_cks.alloc((size_t)m.nnodes))
    return EQLB_ERR_DEVICE;
  double* d_korn = cells_kornconst;
  if (memspace == EQLB_MEM_HOST)
  {
    if (!h->d_korn && h->d_korn.alloc((size_t)m.ncells))
      return EQLB_ERR_DEVICE;
    HIP_TRY(hipMemcpyAsync(h->d_korn, cells_kornconst, sizeof(double) * m.ncells, hipMemcpyHostToDevice, stream));
    d_korn = h->d_korn;
  }
  eqlb::launch_korn(m, h->bt.node_slot, h->bt.node_patch, h->bt.slot_cell, h->bt.slot_info, h->bt.pn, h->bt.pflag,
                    h->d_cks, d_korn, stream, h->bt.l_npatch, h->bt.l_nodes, h->bt.l_off, h->bt.l_slot_cell, h->bt.l_slot_info,
                    h->bt.l_pflag);
  HIP_TRY(hipGetLastError());
  if (memspace == EQLB_MEM_HOST)
  {
    HIP_TRY(hipMemcpyAsync(cells_kornconst, d_korn, sizeof(double) * m.ncells, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
  }
  return EQLB_OK;
}
EQLB_CATCH_ALL

int64_t eqlb_se_num_patches(const eqlb_se_t* h) { return h ? h->bt.npatch_total : 0; }

int eqlb_se_tiling_info(const eqlb_se_t* h, int64_t* ntiles, int64_t* cells_per_tile,
                        int64_t* npatch_instances, int64_t* nlane_slots)
{
  if (!h || !h->bt.boundary_set)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_tiling_info: set the boundary first");
  if (ntiles)
    *ntiles = h->bt.ntiles;
  if (cells_per_tile)
    *cells_per_tile = h->bt.tile_tc;
  if (npatch_instances)
    *npatch_instances = h->bt.t_npatch;
  if (nlane_slots)
    *nlane_slots = h->bt.t_nslots;
  return EQLB_OK;
}

int eqlb_se_tiling_blocks(const eqlb_se_t* h, int64_t* out, int32_t n)
{
  if (!h || !h->bt.boundary_set)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_tiling_blocks: set the boundary first");
  if (n < 0 || (n > 0 && !out))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_tiling_blocks: invalid argument");
  for (int32_t i = 0; i < std::min<int32_t>(n, EQLB_TB_COUNT); ++i)
    out[i] = h->bt.ntiles > 0 ? h->bt.t_blocks[i] : 0;
  return EQLB_OK;
}

int eqlb_se_large_patch_info(const eqlb_se_t* h, int64_t* npatches, int32_t* max_cells)
{
  if (!h || !h->bt.boundary_set)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_large_patch_info: set the boundary first");
  if (npatches)
    *npatches = h->bt.l_npatch;
  if (max_cells)
    *max_cells = h->bt.l_maxcells;
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

int32_t eqlb_se_num_priority_tiles(const eqlb_se_t* h) { return (h && h->bt.boundary_set) ? h->bt.t_nprio : 0; }

int eqlb_se_export_patches(eqlb_se_t* h, int32_t stride, int32_t* ncells, int32_t* cells,
                           int32_t* fcts, int8_t* fcts_local, int8_t* inodes_local,
                           int8_t* reversed)
try
{
  if (!h || !ncells || !cells || !fcts || !fcts_local || !inodes_local || !reversed)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_export_patches: null argument");
  if (!h->bt.boundary_set)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_export_patches: set the boundary first");
  const eqlb::DeviceMesh& m = h->mesh->m;
  if (stride < m.ncells_max + 2)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_export_patches: stride too small");
  const size_t nn = (size_t)m.nnodes;
  eqlb::HostCall s;
  const auto d_n = s.out(ncells, nn), d_c = s.out(cells, nn * stride), d_f = s.out(fcts, nn * stride);
  const auto d_fl = s.out(fcts_local, nn * stride * 2), d_il = s.out(inodes_local, nn * stride),
             d_rv = s.out(reversed, nn * stride * 2);
  if (s.upload(nullptr) == hipSuccess)
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
    a.facet_type = h->bt.facet_type;
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
    s.note(hipGetLastError());
  }
  const hipError_t e = s.finish(nullptr);
  return e == hipSuccess ? EQLB_OK : fail(EQLB_ERR_DEVICE, "eqlb_se_export_patches: %s", hipGetErrorString(e));
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
  const bool host = memspace == EQLB_MEM_HOST;
  eqlb::HostCall s; // (the projection matrix is staged in either memory space)
  const auto d_P = s.in(Pm.data(), Pm.size());
  const auto d_in = s.in(host ? qvalues : nullptr, n_in);
  const auto d_out = s.out(host ? out : nullptr, n_out);
  if (s.upload(stream) == hipSuccess)
  {
    eqlb::launch_project_dg(ncells, nd, nq, bs, d_P, host ? d_in.get() : qvalues, host ? d_out.get() : out, stream);
    s.note(hipGetLastError());
  }
  const hipError_t e = s.finish(stream);
  return e == hipSuccess ? EQLB_OK : fail(EQLB_ERR_DEVICE, "eqlb_project_dg: %s", hipGetErrorString(e));
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
                         double alpha, double beta, const eqlb::EstWeightArgs* weight = nullptr)
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
                                         facet_jump, alpha, beta, stream, weight);
    return st ? fail(st, "eqlb_se_estimate: kernel launch failed") : EQLB_OK;
  }
  EQLB_TRY(eqlb::check_memspace("eqlb_se_estimate", memspace));
  eqlb::HostCall s;
  const auto d_x = s.in(flux_hdiv, n_x), d_g = s.in(flux_dg, n_g), d_f = s.in(rhs_dg, n_f);
  const auto d_d = s.out(cell_div2, n_c), d_s = s.out(cell_sig2, n_c), d_j = s.out(facet_jump, n_e);
  const auto d_wc = s.in(weight ? weight->cell_coeff : nullptr, (size_t)m.ncells),
             d_wd = s.in(weight ? weight->cell_D : nullptr, 3 * (size_t)m.ncells);
  int rc = EQLB_OK;
  if (s.upload(stream) == hipSuccess)
  {
    const eqlb::EstWeightArgs wx{weight && weight->cell_coeff ? d_wc.get() : nullptr,
                                 weight && weight->cell_D ? d_wd.get() : nullptr};
    rc = eqlb::launch_estimate(m, k, degree_dg, nrhs, d_x, d_g, d_f, d_d, d_s, d_j, alpha, beta, stream,
                               weight ? &wx : nullptr);
  }
  if (s.finish(stream) != hipSuccess || rc)
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

// the body of the weighted entries: without a coefficient and a tensor the call of the entry without a weight; host
// arrays are checked cell by cell before anything is launched, device arrays are the caller's responsibility
static int estimate_weighted_call(const char* who, eqlb_mesh_t* mesh, int32_t k, int32_t degree_dg, int32_t nrhs,
                                  const double* flux, const double* flux_dg, const double* rhs_dg,
                                  const double* cell_coeff, const double* cell_D, double* cell_div2, double* cell_sig2,
                                  double* facet_jump, int32_t memspace, void* stream, double alpha, double beta)
{
  if (mesh && memspace == EQLB_MEM_HOST)
    EQLB_TRY(eqlb::check_cells(who, mesh->m.ncells, {{eqlb::CELL_COEFF, cell_coeff}, {eqlb::CELL_D, cell_D}}));
  const eqlb::EstWeightArgs weight{cell_coeff, cell_D};
  return estimate_impl(mesh, k, degree_dg, nrhs, flux, flux_dg, rhs_dg, cell_div2, cell_sig2, facet_jump, memspace,
                       stream, alpha, beta, (cell_coeff || cell_D) ? &weight : nullptr);
}

int eqlb_se_estimate_weighted(eqlb_mesh_t* mesh, int32_t k, int32_t degree_dg, int32_t nrhs, const double* flux_hdiv,
                              const double* flux_dg, const double* rhs_dg, const double* cell_coeff,
                              const double* cell_D, double* cell_div2, double* cell_sig2, double* facet_jump,
                              int32_t memspace, void* stream)
{
  return estimate_weighted_call("eqlb_se_estimate_weighted", mesh, k, degree_dg, nrhs, flux_hdiv, flux_dg, rhs_dg,
                                cell_coeff, cell_D, cell_div2, cell_sig2, facet_jump, memspace, stream, 0.0, 1.0);
}

int eqlb_ev_estimate_weighted(eqlb_mesh_t* mesh, int32_t k, int32_t degree_dg, int32_t nrhs, const double* flux_broken,
                              const double* flux_dg, const double* rhs_dg, const double* cell_coeff,
                              const double* cell_D, double* cell_div2, double* cell_sig2, double* facet_jump,
                              int32_t memspace, void* stream)
{
  return estimate_weighted_call("eqlb_ev_estimate_weighted", mesh, k, degree_dg, nrhs, flux_broken, flux_dg, rhs_dg,
                                cell_coeff, cell_D, cell_div2, cell_sig2, facet_jump, memspace, stream, -1.0, 0.0);
}

// the body of eqlb_se_estimate_stress and eqlb_se_estimate_stress_mu; co: the cell-wise coefficients of the latter, its
// arrays in `memspace`, or nullptr (the scalar pi_1, mu = 1)
static int estimate_stress_call(const char* who, eqlb_mesh_t* mesh, int32_t k, const double* flux_hdiv,
                                const double* korn, double pi_1, const eqlb::StressCoeffArgs* co, double* cell_energy,
                                double* cell_wsym, double* node_asym, int32_t memspace, void* stream_)
{
  if (!mesh || !flux_hdiv || k < 1 || k > 4 || !(pi_1 > -1.0))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: invalid argument", who);
  EQLB_TRY(eqlb::check_memspace(who, memspace));
  const eqlb::DeviceMesh& m = mesh->m;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (co && memspace == EQLB_MEM_HOST)
    EQLB_TRY(eqlb::check_cells(who, m.ncells, {{eqlb::CELL_MU, co->cell_mu}, {eqlb::CELL_PI1, co->cell_pi1}}));
  const int32_t* node_cells = nullptr; // (first use from several threads: the handle's lock is taken there)
  if (node_asym && eqlb::mesh_node_cells(mesh, &node_cells))
    return fail(EQLB_ERR_DEVICE, "%s: device allocation failed", who);
  const size_t nx = (size_t)m.ncells * k * (k + 2);
  int rc;
  if (memspace == EQLB_MEM_DEVICE)
    rc = eqlb::launch_estimate_stress(m, node_cells, k, flux_hdiv, flux_hdiv + nx, korn, pi_1, cell_energy,
                                      cell_wsym, node_asym, stream, co);
  else
  {
    eqlb::HostCall s;
    const auto d_x = s.in(flux_hdiv, 2 * nx), d_k = s.in(korn, m.ncells);
    const auto d_p = s.in(co ? co->cell_pi1 : nullptr, m.ncells), d_m = s.in(co ? co->cell_mu : nullptr, m.ncells);
    const auto d_e = s.out(cell_energy, m.ncells), d_w = s.out(cell_wsym, m.ncells), d_a = s.out(node_asym, m.nnodes);
    if (s.upload(stream) != hipSuccess)
      return fail(EQLB_ERR_DEVICE, "%s: device allocation failed", who);
    eqlb::StressCoeffArgs dco;
    if (co)
      dco = eqlb::StressCoeffArgs{co->cell_pi1 ? d_p.get() : nullptr, co->cell_mu ? d_m.get() : nullptr, co->pi_1, co->mu};
    rc = eqlb::launch_estimate_stress(m, node_cells, k, d_x, d_x + nx, d_k, pi_1, d_e, d_w, d_a, stream,
                                      co ? &dco : nullptr);
    if (s.finish(stream) != hipSuccess)
      rc = EQLB_ERR_DEVICE;
  }
  return rc ? fail(rc, "%s: device error", who) : EQLB_OK;
}

int eqlb_se_estimate_stress(eqlb_mesh_t* mesh, int32_t k, const double* flux_hdiv, const double* korn,
                            double pi_1, double* cell_energy, double* cell_wsym, double* node_asym,
                            int32_t memspace, void* stream)
{
  return estimate_stress_call("eqlb_se_estimate_stress", mesh, k, flux_hdiv, korn, pi_1, nullptr, cell_energy, cell_wsym,
                              node_asym, memspace, stream);
}

int eqlb_se_estimate_stress_mu(eqlb_mesh_t* mesh, int32_t k, const double* flux_hdiv, const double* korn, double pi_1,
                               const double* cell_pi1, double mu, const double* cell_mu, double* cell_energy,
                               double* cell_wsym, double* node_asym, int32_t memspace, void* stream)
{
  const char* who = "eqlb_se_estimate_stress_mu";
  if (!cell_mu)
    EQLB_TRY(eqlb::check_scalar(who, "mu", *eqlb::CELL_MU.rule, mu));
  const eqlb::StressCoeffArgs co{cell_pi1, cell_mu, pi_1, mu};
  const bool plain = !cell_pi1 && !cell_mu && mu == 1.0; // the kernel of eqlb_se_estimate_stress
  return estimate_stress_call(who, mesh, k, flux_hdiv, korn, cell_pi1 ? 0.0 : pi_1, plain ? nullptr : &co, cell_energy,
                              cell_wsym, node_asym, memspace, stream);
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
  EQLB_TRY(eqlb::check_memspace("eqlb_oscillation", memspace));
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
    eqlb::HostCall s;
    const auto d_x = s.in(flux, nx), d_g = s.in(flux_dg, ng), d_f = s.in(fvalues, (size_t)nrhs * m.ncells * nq),
               d_k = s.in(korn, m.ncells);
    const auto d_o = s.out(out, (size_t)nrhs * m.ncells);
    if (s.upload(stream) != hipSuccess)
      return fail(EQLB_ERR_DEVICE, "eqlb_oscillation: device allocation failed");
    rc = eqlb::launch_oscillation(m, k, degree_dg, nrhs, d_x, d_g, nq, qpoints, qweights, d_f, d_k, d_o, stream);
    if (s.finish(stream) != hipSuccess)
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
  EQLB_TRY(eqlb::check_memspace("eqlb_boundary_residual", memspace));
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
    eqlb::HostCall s;
    const auto d_x = s.in(flux, nx), d_g = s.in(flux_dg, ng), d_b = s.in(boundary_values, nx);
    const auto d_l = s.in(facets, (size_t)nfacets_bc);
    const auto d_o = s.out(out, (size_t)nrhs * nfacets_bc);
    rc = EQLB_OK;
    if (s.upload(stream) == hipSuccess)
      rc = eqlb::launch_boundary_residual(m, k, degree_dg, nrhs, d_x, d_g, nfacets_bc, d_l, d_b, d_o, stream);
    if (s.finish(stream) != hipSuccess)
      rc = EQLB_ERR_DEVICE;
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
  std::unique_ptr<eqlb_ev> h(new eqlb_ev());
  eqlb_se* se = nullptr;
  EQLB_TRY(eqlb_se_create(mesh, k, degree_dg, nrhs, 0, 0, &se));
  h->se.reset(se);
  se->mode = 1;
  se->ev_ndofs = (int64_t)mesh->m.nfacets * k + (int64_t)mesh->m.ncells * (k * k - k);
  *handle = h.release();
  return EQLB_OK;
}
EQLB_CATCH_ALL

void eqlb_ev_destroy(eqlb_ev_t* h) { delete h; }

int eqlb_ev_set_option(eqlb_ev_t* h, const char* key, int32_t value)
{
  if (!h || !key)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_ev_set_option: null argument");
  if (!strcmp(key, "output"))
  {
    if (value != 0 && value != 1)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "unknown output layout %d", value);
    h->se->ev_output = value;
    h->se->d_flux_hdiv.reset(); // staging size depends on the layout
    h->se->d_flux_dg.reset();
    h->se->d_rhs_dg.reset();
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
    return eqlb_se_set_option(h->se.get(), key, value);
  return fail(EQLB_ERR_INVALID_ARGUMENT, "unknown option '%s'", key);
}

int eqlb_ev_set_dofmap(eqlb_ev_t* h, const int32_t* cell_dofs, int64_t ndofs)
try
{
  if (!h)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_ev_set_dofmap: null argument");
  eqlb_se* se = h->se.get();
  const eqlb::DeviceMesh& m = se->mesh->m;
  se->ev_cell_dofs.reset();
  se->d_flux_hdiv.reset(); // staging size depends on the number of DOFs
  se->d_flux_dg.reset();
  se->d_rhs_dg.reset();
  if (!cell_dofs)
  {
    se->ev_ndofs = (int64_t)m.nfacets * se->k + (int64_t)m.ncells * (se->k * se->k - se->k);
    return EQLB_OK;
  }
  const size_t n = (size_t)m.ncells * se->nrt;
  for (size_t i = 0; i < n; ++i)
    if (cell_dofs[i] < 0 || cell_dofs[i] >= ndofs)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_ev_set_dofmap: DOF %d out of range", cell_dofs[i]);
  if (se->ev_cell_dofs.upload(cell_dofs, n))
    return EQLB_ERR_DEVICE;
  se->ev_ndofs = ndofs;
  return EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_ev_set_basis_transform(eqlb_ev_t* h, const double* C, const double* R)
{
  if (!h)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_ev_set_basis_transform: null argument");
  eqlb_se* se = h->se.get();
  se->ev_basis.reset();
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
  if (se->ev_basis.upload(buf.data(), buf.size()))
    return EQLB_ERR_DEVICE;
  se->ev_basis_has_R = R != nullptr;
  return EQLB_OK;
}

int64_t eqlb_ev_num_dofs(const eqlb_ev_t* h) { return h ? h->se->ev_ndofs : 0; }

int64_t eqlb_ev_num_patches(const eqlb_ev_t* h) { return h ? h->se->bt.npatch_total : 0; }

int eqlb_ev_large_patch_info(const eqlb_ev_t* h, int64_t* npatches, int32_t* max_cells)
{
  if (!h)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_ev_large_patch_info: null handle");
  return eqlb_se_large_patch_info(h->se.get(), npatches, max_cells);
}

int eqlb_ev_tiling_blocks(const eqlb_ev_t* h, int64_t* out, int32_t n)
{
  if (!h)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_ev_tiling_blocks: null handle");
  return eqlb_se_tiling_blocks(h->se.get(), out, n);
}

} // extern "C"
