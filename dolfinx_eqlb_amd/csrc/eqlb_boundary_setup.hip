// Driver of the set-up behind eqlb_se_set_boundary / eqlb_ev_set_boundary.  The call is planned on the host first
// (plan_boundary of eqlb_boundary_plan.h, plan_tiles of eqlb_tiling_host.hip): neither touches the handle, and every
// refusal that depends on the arguments, the mesh and the options alone happens there - a refused call leaves the
// handle as it was.  Then the old boundary tables are dropped and the new ones built step by step: uploads and launches
// of the patch builder.  Only a device error (allocation, fill, builder launch) can leave a handle without tables:
// boundary_set stays false, the next eqlb_se_set_boundary or the end of the handle cleans up.
#include "eqlb_handle.h"

#include <algorithm>

namespace
{
using eqlb::BoundaryPlan;
using eqlb::BoundaryTables;
using eqlb::DevBuf;

eqlb::HostTopology host_topology(const eqlb_mesh& mesh)
{
  const eqlb::DeviceMesh& m = mesh.m;
  const eqlb::HostMesh& h = mesh.host;
  return {m.nnodes, m.ncells, m.nfacets, h.node_ncells.data(), h.node_nfcts.data(), h.node_nbnd.data(),
          h.cell_nodes.data(), h.facet_nodes.data(), h.facet_cells_off.data(), h.node_facets_off.data(),
          h.node_facets.data(), h.node_cells_off.data(), h.node_cells.data()};
}

// arguments of the patch builder that every SoA of the handle shares: the mesh and the facet types
eqlb::BuildArgs builder_args(const eqlb_se* h)
{
  const eqlb::DeviceMesh& m = h->mesh->m;
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
  a.node_ws = h->bt.node_ws;
  a.node_group = h->bt.node_group;
  a.node_wslevel = h->bt.node_wslevel;
  return a;
}

// The plain SoA: one patch per equilibrated node of the bins, lane slots bin by bin
int build_plain_soa(eqlb_se* h, const BoundaryPlan& p, const int8_t* facet_type, const double* boundary_values)
{
  const eqlb::DeviceMesh& m = h->mesh->m;
  BoundaryTables& t = h->bt;
  t.stress_flux_bcs = p.stress_flux_bcs;
  t.nslots = p.nslots;
  t.npatch_total = p.npatch_total;
  std::copy(p.bins, p.bins + eqlb::MAX_BINS, t.bins);
  int st = 0;
  st |= t.facet_type.upload(facet_type, (size_t)h->nrhs * m.nfacets);
  if (p.inhomogeneous)
    st |= t.bvals.upload(boundary_values, (size_t)h->nrhs * m.ncells * h->nrt);
  st |= t.node_slot.upload(p.node_slot.data(), (size_t)m.nnodes);
  st |= t.node_patch.upload(p.node_patch.data(), (size_t)m.nnodes);
  st |= t.slot_cell.alloc((size_t)t.nslots);
  st |= t.slot_info.alloc((size_t)t.nslots);
  st |= t.pn.alloc((size_t)t.npatch_total);
  st |= t.pflag.alloc((size_t)t.npatch_total * h->nrhs);
  if (st)
    return EQLB_ERR_DEVICE;
  HIP_TRY(hipMemset(t.slot_cell, 0xff, sizeof(int32_t) * std::max<int64_t>(t.nslots, 1)));
  HIP_TRY(hipMemset(t.slot_info, 0, sizeof(uint32_t) * std::max<int64_t>(t.nslots, 1)));
  if (p.any)
  {
    t.ws_levels = p.ws_levels;
    if (t.node_ws.upload(p.ws.data(), p.ws.size()) || t.node_group.upload(p.group.data(), p.group.size())
        || t.node_wslevel.upload(p.level.data(), p.level.size()))
      return EQLB_ERR_DEVICE;
  }
  eqlb::BuildArgs a = builder_args(h);
  a.node_slot = t.node_slot;
  a.node_patch = t.node_patch;
  a.npatch_total = t.npatch_total;
  a.slot_cell = t.slot_cell;
  a.slot_info = t.slot_info;
  a.pn = t.pn;
  a.pflag = t.pflag;
  eqlb::launch_build_patches(a, nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  return EQLB_OK;
}

// The large patches: lane slots in CSR form (l_off), the same descriptor bits, flags per right-hand side
int build_large_soa(eqlb_se* h, const BoundaryPlan& p)
{
  const eqlb::DeviceMesh& m = h->mesh->m;
  BoundaryTables& t = h->bt;
  const int64_t nl = (int64_t)p.large_nodes.size(), nslots = p.l_off[nl];
  t.l_maxcells = p.l_maxcells;
  std::vector<int64_t> lslot(m.nnodes, -1), lpatch(m.nnodes, -1);
  for (int64_t q = 0; q < nl; ++q)
  {
    lslot[p.large_nodes[q]] = p.l_off[q];
    lpatch[p.large_nodes[q]] = q;
  }
  DevBuf<int64_t> d_lslot, d_lpatch;
  int st = 0;
  st |= t.l_off.upload(p.l_off.data(), p.l_off.size());
  st |= t.l_slot_cell.alloc((size_t)nslots);
  st |= t.l_slot_info.alloc((size_t)nslots);
  st |= t.l_pflag.alloc((size_t)nl * h->nrhs);
  st |= t.l_cells.upload(p.l_cells.data(), p.l_cells.size());
  st |= t.l_ws.alloc(eqlb::large_patch_ws_doubles(h->k, nslots, nl));
  st |= t.l_nodes.upload(p.large_nodes.data(), p.large_nodes.size());
  if (h->stress)
  {
    st |= t.l_wsym_off.upload(p.l_wsym_off.data(), (size_t)nl);
    st |= t.l_wsym_ws.alloc((size_t)p.l_wsym_off[nl]);
  }
  st |= d_lslot.upload(lslot.data(), lslot.size());
  st |= d_lpatch.upload(lpatch.data(), lpatch.size());
  if (st)
    return EQLB_ERR_DEVICE;
  eqlb::BuildArgs a = builder_args(h);
  a.node_ws = nullptr;
  a.node_slot = d_lslot;
  a.node_patch = d_lpatch;
  a.npatch_total = nl;
  a.slot_cell = t.l_slot_cell;
  a.slot_info = t.l_slot_info;
  a.pn = nullptr;
  a.pflag = t.l_pflag;
  a.large = 1;
  eqlb::launch_build_patches(a, nullptr);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess)
    e = hipDeviceSynchronize();
  if (e != hipSuccess)
    return fail(EQLB_ERR_DEVICE, "large-patch builder: %s", hipGetErrorString(e));
  t.l_npatch = nl;
  t.l_nslots = nslots;
  t.l_ncells = (int64_t)p.l_cells.size();
  t.l_stress = h->large_patches_stress != 0;
  return EQLB_OK;
}

// The tiled SoA: the tiles and their cells as planned, the patch instances by the builder; EV mode: the table of the
// facets that a tile flushes to the conforming DOFs
int build_tiled_soa(eqlb_se* h, const BoundaryPlan& p, const eqlb::TilePlan& tp)
{
  SetupTimer tm;
  BoundaryTables& t = h->bt;
  t.t_mixed = p.t_mixed;
  t.t_rest = p.t_rest;
  t.t_nprio = tp.nprio;
  std::copy(tp.blocks, tp.blocks + EQLB_TB_COUNT, t.t_blocks);
  t.ntiles = tp.ntiles;
  t.tile_tc = tp.tc;
  t.t_nslots = tp.nslots;
  t.t_npatch = (int64_t)tp.inst_node.size();
  const size_t nslots = (size_t)std::max<int64_t>(tp.nslots, 1);
  DevBuf<int32_t> d_inode, d_islot, d_itile, d_ctile, d_cpos;
  int st = 0;
  st |= t.t_tiles.upload(tp.tiles.data(), tp.tiles.size());
  st |= t.t_tile_cells.upload(tp.tile_cells.data(), tp.tile_cells.size());
  st |= t.t_slot_cell.alloc(nslots);
  st |= t.t_slot_info.alloc(nslots);
  st |= t.t_pn.alloc((size_t)t.t_npatch);
  st |= t.t_pflag.alloc((size_t)std::max<int64_t>(t.t_npatch, 1) * h->nrhs);
  st |= d_inode.upload(tp.inst_node.data(), tp.inst_node.size());
  st |= d_islot.upload(tp.inst_slot.data(), tp.inst_slot.size());
  st |= d_itile.upload(tp.inst_tile.data(), tp.inst_tile.size());
  st |= d_ctile.upload(tp.cell_tile.data(), tp.cell_tile.size());
  st |= d_cpos.upload(tp.cell_pos.data(), tp.cell_pos.size());
  if (st)
    return EQLB_ERR_DEVICE;
  hipError_t e = hipMemset(t.t_slot_cell, 0xff, sizeof(int32_t) * nslots);
  if (e == hipSuccess)
    e = hipMemset(t.t_slot_info, 0, sizeof(uint32_t) * nslots);
  eqlb::BuildArgs a = builder_args(h);
  a.ninst = t.t_npatch;
  a.inst_node = d_inode;
  a.inst_slot = d_islot;
  a.inst_tile = d_itile;
  a.cell_tile = d_ctile;
  a.cell_pos = d_cpos;
  a.tile_cells = tp.tc;
  a.node_slot = t.node_slot;
  a.node_patch = t.node_patch;
  a.npatch_total = t.t_npatch;
  a.slot_cell = t.t_slot_cell;
  a.slot_info = t.t_slot_info;
  a.pn = t.t_pn;
  a.pflag = t.t_pflag;
  if (e == hipSuccess && a.ninst > 0)
  {
    eqlb::launch_build_patches(a, nullptr);
    e = hipGetLastError();
  }
  if (e == hipSuccess)
    e = hipDeviceSynchronize();
  tm.lap("tiles: upload + builder kernel");
  if (e != hipSuccess)
    return fail(EQLB_ERR_DEVICE, "tiled patch builder: %s", hipGetErrorString(e));
  if (h->mode == 1)
  {
    const int64_t ne = (int64_t)t.ntiles * t.tile_tc * 3;
    if (t.t_facet_owner.alloc((size_t)ne))
      return EQLB_ERR_DEVICE;
    eqlb::launch_tile_facet_owner(h->mesh->m, ne, t.t_tile_cells, t.t_facet_owner, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
  }
  return EQLB_OK;
}

// Fused stress launch: the cells of the compact reduction behind it - those of the rest, and with large patches the
// merged list of both
int upload_rest_cells(eqlb_se* h, const BoundaryPlan& p)
{
  BoundaryTables& t = h->bt;
  t.nrest_cells = (int64_t)p.rest_cells.size();
  if (!p.rest_cells.empty() && t.rest_cells.upload(p.rest_cells.data(), p.rest_cells.size()))
    return EQLB_ERR_DEVICE;
  if (p.t_stress && t.l_npatch > 0)
  {
    t.l_nrest_cells = (int64_t)p.l_rest_cells.size();
    if (t.l_rest_cells.upload(p.l_rest_cells.data(), p.l_rest_cells.size()))
      return EQLB_ERR_DEVICE;
  }
  return EQLB_OK;
}

} // namespace

extern "C" {

int eqlb_se_set_boundary(eqlb_se_t* h, const int8_t* facet_type, const double* boundary_values,
                         const uint8_t* node_mask)
try
{
  if (!h || !facet_type)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_set_boundary: null argument");
  SetupTimer tm;
  const eqlb::PlanOptions opt{h->k, h->deg, h->nrhs, h->nrt, h->stress, h->mode, h->large_patches,
                              h->large_patches_stress, eqlb::large_patch_weaksym_ws_doubles};
  const eqlb::HostTopology topo = host_topology(*h->mesh);
  // A cell of zero area: the patches of its three vertices are left out like masked nodes, and every sweep reports
  // them through the status word (flat_swept).  Inside a patch kernel their inf and NaN would not stay in their own
  // lanes - the chains of the shuffle solver multiply what they drag in from the neighbouring patch group by an exact
  // zero, which is no zero for a NaN -, and RT_1 has no pivot that could report them
  const uint8_t* flat = nullptr;
  EQLB_TRY(eqlb::mesh_flat_nodes(h->mesh, &flat));
  std::vector<uint8_t> healthy_mask;
  bool flat_swept = false;
  if (flat)
  {
    healthy_mask.resize((size_t)topo.nnodes);
    for (int32_t i = 0; i < topo.nnodes; ++i)
    {
      const bool asked = !node_mask || node_mask[i];
      flat_swept = flat_swept || (asked && flat[i]);
      healthy_mask[i] = (asked && !flat[i]) ? 1 : 0;
    }
    node_mask = healthy_mask.data();
  }
  BoundaryPlan plan; // (plan_boundary, in its two halves)
  int st = eqlb::check_boundary_table(topo, opt, facet_type, node_mask, plan);
  tm.lap("checks");
  if (!st)
    st = eqlb::plan_patches(topo, opt, facet_type, boundary_values, node_mask, plan);
  if (st)
    return fail(st, "%s", plan.message.c_str());
  tm.lap("binning"); // (with the groups and the large patches of a stress handle)
  eqlb::TilePlan tiles;
  if (plan.tiles)
    EQLB_TRY(eqlb::plan_tiles(h, plan, tiles));
  tm.lap("tiles: plan (total)");

  h->bt = BoundaryTables{}; // (the slot buffer as well: re-zeroed by the next sweep, node_mask may have changed)
  h->bt.t_stress = plan.t_stress;
  h->bt.flat_swept = flat_swept;
  tm.lap("free old tables");
  EQLB_TRY(build_plain_soa(h, plan, facet_type, boundary_values));
  tm.lap("plain SoA: upload + builder");
  if (!plan.large_nodes.empty())
  {
    EQLB_TRY(build_large_soa(h, plan));
    tm.lap("large-patch SoA");
  }
  if (plan.tiles)
    EQLB_TRY(build_tiled_soa(h, plan, tiles));
  EQLB_TRY(upload_rest_cells(h, plan));
  tm.lap("tiles (total)"); // (what is left of them behind the plan: uploads, builder, EV facet owners, rest cells)
  h->bt.boundary_set = true;
  return EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_ev_set_boundary(eqlb_ev_t* h, const int8_t* facet_type, const double* boundary_values,
                         const uint8_t* node_mask)
try
{
  if (!h)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_ev_set_boundary: null argument");
  eqlb_se* se = h->se.get();
  EQLB_TRY(eqlb_se_set_boundary(se, facet_type, nullptr, node_mask));
  const eqlb::DeviceMesh& m = se->mesh->m;
  bool inhomogeneous = false;
  const size_t nb = (size_t)se->nrhs * se->ev_ndofs;
  if (boundary_values)
    for (size_t i = 0; i < nb && !inhomogeneous; ++i)
      inhomogeneous = (boundary_values[i] != 0.0);
  if (!inhomogeneous)
    return EQLB_OK;
  // conforming boundary DOFs -> the broken per-cell layout the patch kernel reads
  const size_t nbroken = (size_t)se->nrhs * m.ncells * se->nrt;
  DevBuf<double> d_conf;
  if (d_conf.upload(boundary_values, nb) || se->bt.bvals.alloc(nbroken))
    return EQLB_ERR_DEVICE;
  hipError_t e = hipMemset(se->bt.bvals, 0, sizeof(double) * nbroken);
  if (e == hipSuccess)
  {
    const double* facet_maps = (se->ev_basis && !se->ev_bv_hier) ? se->ev_basis + se->nrt * se->nrt + se->k * se->k : nullptr;
    eqlb::launch_ev_boundary_to_broken(m, se->k, se->nrhs, se->ev_cell_dofs, se->ev_ndofs, d_conf, se->bt.bvals, facet_maps,
                                       nullptr);
    e = hipDeviceSynchronize();
  }
  if (e != hipSuccess)
    return fail(EQLB_ERR_DEVICE, "eqlb_ev_set_boundary: %s", hipGetErrorString(e));
  return EQLB_OK;
}
EQLB_CATCH_ALL

} // extern "C"
