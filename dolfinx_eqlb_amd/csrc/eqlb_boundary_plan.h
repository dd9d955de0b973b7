// Planner of eqlb_se_set_boundary: everything that call decides from its arguments, the host copies of the mesh and the
// options of the handle - the checks, the bins, the order of the patches inside a bin, the large patches, the groups of
// boundary patches of the stress path, what the tiles list - computed into a BoundaryPlan.  It writes nothing but that
// plan and calls nothing of HIP: eqlb_boundary_setup.hip runs it BEFORE the handle changes, so a refused table leaves
// the handle as it was, and the stand-alone host program tools/boundary_plan_emul.cpp includes this file with a plain
// C++ compiler.  The bins and limits it shares with the kernels are in eqlb_bins.h.
#pragma once

#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/eqlb.h"
#include "eqlb_bins.h"
#include "eqlb_topology_check.h"

namespace eqlb
{

// The host copies of the mesh, kept by the mesh handle for the planners (boundary plan, tiling, the boundary-facet checks
// of the update and carry entries, the lengths of eqlb_mesh_export).  Filled once by the creator of the handle
struct HostMesh
{
  std::vector<int32_t> node_ncells, node_nfcts, node_nbnd;       // cells / facets / one-cell facets at each node
  std::vector<int32_t> cell_nodes, facet_nodes, facet_cells_off; // [ncells][3], [nfacets][2], [nfacets + 1]
  std::vector<int32_t> node_facets_off, node_facets, node_cells_off, node_cells; // CSR
  std::vector<double> x;                                         // [nnodes][3]
};

// What the planner reads of them (host_topology of eqlb_boundary_setup.hip; the stand-alone programs fill their own)
struct HostTopology
{
  int32_t nnodes, ncells, nfacets;
  const int32_t *node_ncells, *node_nfcts, *node_nbnd; // cells / facets / one-cell facets at each node
  const int32_t* cell_nodes;                           // [ncells][3]
  const int32_t *facet_nodes, *facet_cells_off;        // [nfacets][2], [nfacets + 1]
  const int32_t *node_facets_off, *node_facets, *node_cells_off, *node_cells; // CSR
};

// The options of the handle that the plan depends on
struct PlanOptions
{
  int k, deg, nrhs, nrt;
  int stress, mode; // mode 1: constrained minimisation (EV)
  int large_patches, large_patches_stress;
  // doubles of weak-symmetry work space of a large patch of n cells (large_patch_weaksym_ws_doubles), nullptr: none
  size_t (*large_wsym_doubles)(int k, int64_t ncells_of_patch);
};

// "interior, as many cells as lanes": the patches that the full-patch instances of the kernels take
inline bool patch_is_full(int32_t ncells, int32_t nfacets, int bin)
{
  return bin >= 0 && ncells == nfacets && ncells == BIN_P[bin];
}

// The cells with a vertex in a flagged node set, ascending (the cell list of a compact reduction)
inline std::vector<int32_t> cells_touching(const int32_t* cell_nodes, int32_t ncells, const std::vector<uint8_t>& flag)
{
  std::vector<int32_t> out;
  for (int32_t c = 0; c < ncells; ++c)
    if (flag[cell_nodes[3 * (size_t)c]] || flag[cell_nodes[3 * (size_t)c + 1]] || flag[cell_nodes[3 * (size_t)c + 2]])
      out.push_back(c);
  return out;
}

// cells per tile that the LDS of a workgroup holds (tile_cells_of, tile_cells_ev_of, tile_cells_max_of of
// eqlb_se_kernels.hip): default, EV mode of RT_3, upper limit
struct TileSizes
{
  int dflt, ev, max;
};

// Tile size: the default, or - on meshes that fill the chip several times over - the size that makes the tiles fill
// whole rounds of the resident workgroup slots: 1M triangles in 2 045 tiles of 489 cells run in 4 rounds of 512, 2 084
// tiles of 480 cells leave 36 tiles for a fifth.  tc_fixed > 0 (fused stress launch: the largest tile its LDS holds):
// ONE workgroup per CU, where a partial last round of the 256 slots costs a full round.
inline int choose_tile_cells(int k, int mode, int64_t ncells, int tc_fixed, int tile_cells_user, const TileSizes& ts)
{
  const bool ev3 = mode == 1 && k >= 3; // EV mode of RT_3 stages 7 KB more tensors: smaller tiles
  // resident workgroup slots of the chip: two per CU for k <= 2, one for k = 3 and for the fused stress launch
  const int64_t slots = (tc_fixed <= 0 && k <= 2) ? 512 : 256;
  const int64_t tcmax = tc_fixed > 0 ? tc_fixed : (ev3 ? ts.ev : ts.max);
  int tc = tc_fixed > 0 ? (int)std::min<int64_t>(tcmax, 448) : (ev3 ? ts.ev : ts.dflt);
  if (ncells >= slots * 256)
  {
    const int64_t rounds = (ncells + slots * tcmax - 1) / (slots * tcmax);
    tc = (int)((ncells + rounds * slots - 1) / (rounds * slots));
  }
  if (tile_cells_user > 0) // tuning knob (option "tile_cells"), capped by what the LDS of a workgroup holds
    tc = (int)std::min<int64_t>(tile_cells_user, tcmax);
  return tc;
}

struct BoundaryPlan
{
  std::string message; // text of the refusal when plan_boundary does not return EQLB_OK
  bool inhomogeneous = false;   // some boundary value is not zero
  bool stress_flux_bcs = false; // some facet of stress row 0 / 1 carries a flux BC
  bool stress_fused_ok = false; // RT_2 stress with DG_1 data and no such facet: the fused tiled launch applies
  // bins by lanes per patch: P = smallest of {4, 8, 16, 32, 64} >= number of patch facets
  std::vector<int8_t> node_bin;                // -1: masked out or a large patch
  std::vector<int64_t> node_slot, node_patch;  // first lane slot / patch index, -1: not in the bins
  Bin bins[MAX_BINS];
  int64_t nslots = 0, npatch_total = 0;
  // patches of more than 63 cells or more than 64 facets (option "large_patches"): lane slots in CSR form
  std::vector<int32_t> large_nodes, l_off; // ascending nodes; [large_nodes.size() + 1] first lane slot
  int32_t l_maxcells = 0;
  std::vector<int32_t> l_cells;    // cells with a vertex whose patch is a large one
  std::vector<int64_t> l_wsym_off; // [large_nodes.size() + 1] first double of the weak-symmetry work space (stress)
  // grouped boundary patches of the stress path (find_stress_groups); empty vectors where the path does not apply
  std::vector<int8_t> ws, level;
  std::vector<int32_t> group;
  int ws_levels = 1;
  bool any = false;
  // tiles: built at all / for the fused stress launch (bins 0, 1 only) / listing every patch of those bins, not the
  // full ones only
  bool tiles = false, t_stress = false, t_mixed = false;
  std::vector<int8_t> tile_bin; // node_bin, -1 where the tiles leave the node to another path (the REST)
  int64_t t_rest = 0;           // patches of the rest
  std::vector<int32_t> rest_cells;   // cells with a vertex of the rest ...
  std::vector<int32_t> l_rest_cells; // ... or of a large patch (fused stress launch with large patches)
};

// message of a refusal + the code back
inline int refuse(BoundaryPlan& p, int code, const char* fmt, ...)
{
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  p.message = buf;
  return code;
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
// p.ws_levels: the number of levels, p.any: a group exists.
inline int find_stress_groups(const HostTopology& m, const int8_t* facet_type, const uint8_t* node_mask,
                              BoundaryPlan& p)
{
  const int32_t nn = m.nnodes;
  std::vector<int8_t>& ws = p.ws;
  std::vector<int32_t>& group = p.group;
  ws.assign(nn, 0);
  group.assign(nn, -1);
  p.any = false;
  std::vector<int8_t> cnt(nn, 0);
  for (int r = 0; r < 2; ++r)
    for (int32_t f = 0; f < m.nfacets; ++f)
      if (facet_type[(size_t)r * m.nfacets + f] == EQLB_FACET_ESSNT_DUAL)
      {
        ++cnt[m.facet_nodes[2 * (size_t)f]];
        ++cnt[m.facet_nodes[2 * (size_t)f + 1]];
      }
  int32_t ngroups = 0;
  for (int32_t node = 0; node < nn; ++node)
  {
    if (node_mask && !node_mask[node])
      continue;
    if (cnt[node] != 4 || group[node] >= 0 || m.node_ncells[node] != 2)
      continue;
    int32_t inner = -1;
    for (int32_t q = m.node_facets_off[node]; q < m.node_facets_off[node + 1] && inner < 0; ++q)
    {
      const int32_t f = m.node_facets[q];
      if (facet_type[f] == EQLB_FACET_INTERNAL)
        inner = (m.facet_nodes[2 * (size_t)f] == node) ? m.facet_nodes[2 * (size_t)f + 1]
                                                       : m.facet_nodes[2 * (size_t)f];
    }
    if (inner < 0)
      continue;
    std::vector<int32_t> members{inner};
    for (int32_t q = m.node_cells_off[inner]; q < m.node_cells_off[inner + 1]; ++q)
      for (int v = 0; v < 3; ++v)
      {
        const int32_t pnt = m.cell_nodes[3 * (size_t)m.node_cells[q] + v];
        if (cnt[pnt] == 4 && m.node_ncells[pnt] == 2
            && std::find(members.begin(), members.end(), pnt) == members.end())
          members.push_back(pnt);
      }
    if (members.size() < 2)
      continue;
    for (int32_t nd : members)
    {
      if (group[nd] >= 0 || (node_mask && !node_mask[nd]))
        return refuse(p, EQLB_ERR_UNSUPPORTED, "Incompatible mesh! To many patches with 2 cells on neumann boundary.");
      group[nd] = ngroups;
      ws[nd] = (nd == inner) ? 2 : 1;
    }
    ++ngroups;
    p.any = true;
  }
  // levels of overlapping groups (ascending group id = the reference's order)
  p.level.assign(nn, 0);
  p.ws_levels = 1;
  if (!p.any)
    return EQLB_OK;
  std::vector<int32_t> inner_of(ngroups, -1);
  for (int32_t node = 0; node < nn; ++node)
    if (ws[node] == 2)
      inner_of[group[node]] = node;
  std::vector<int> glevel(ngroups, 0);
  for (int32_t g = 0; g < ngroups; ++g)
  {
    const int32_t node = inner_of[g];
    int lv = 0;
    for (int32_t q = m.node_cells_off[node]; q < m.node_cells_off[node + 1]; ++q)
      for (int v = 0; v < 3; ++v)
      {
        const int32_t nd = m.cell_nodes[3 * (size_t)m.node_cells[q] + v];
        if (group[nd] >= 0 && group[nd] < g)
          lv = std::max(lv, glevel[group[nd]] + 1);
      }
    glevel[g] = lv;
    p.ws_levels = std::max(p.ws_levels, lv + 1);
  }
  if (p.ws_levels > WS_MAX_LEVELS)
    return refuse(p, EQLB_ERR_UNSUPPORTED, "more than %d levels of overlapping groups of boundary patches",
                  WS_MAX_LEVELS);
  for (int32_t node = 0; node < nn; ++node)
    if (group[node] >= 0)
      p.level[node] = (int8_t)glevel[group[node]];
  return EQLB_OK;
}

// The facet types, the nodes and what the patch builder cannot walk (eqlb_topology_check.h).  Facets both of whose
// nodes are masked out are not looked at.
inline int check_boundary_table(const HostTopology& m, const PlanOptions& o, const int8_t* facet_type,
                                const uint8_t* node_mask, BoundaryPlan& p)
{
  for (size_t i = 0; i < (size_t)o.nrhs * m.nfacets; ++i)
    if (facet_type[i] < EQLB_FACET_INTERNAL || facet_type[i] > EQLB_FACET_ESSNT_DUAL)
      return refuse(p, EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_set_boundary: facet type %d out of range",
                    (int)facet_type[i]);
  // OrientedPatch::set_max_patch_size (se/Patch.cpp:337-404): every local node is checked
  for (int32_t i = 0; i < m.nnodes; ++i)
  {
    if (node_mask && !node_mask[i])
      continue; // the reference loops the owned nodes only (size_local)
    if (m.node_ncells[i] == 1)
      return refuse(p, EQLB_ERR_PATCH_TOO_SMALL, "Patch around node %d has only 1 cells.", i);
    if (m.node_ncells[i] < 1)
      return refuse(p, EQLB_ERR_INVALID_ARGUMENT, "node %d belongs to no cell", i);
  }
  const TopoFinding tf = check_boundary_topology(m.nnodes, m.nfacets, o.nrhs, m.node_ncells, m.node_nfcts, m.node_nbnd,
                                                 m.facet_nodes, m.facet_cells_off, facet_type, node_mask);
  if (tf.verdict == TOPO_NODE_NOT_WALKABLE)
    return refuse(p, EQLB_ERR_UNSUPPORTED,
                  "Patch around node %d (%d cells, %d facets, %d of them boundary facets) is neither one closed ring nor "
                  "one open fan of cells: a vertex where the boundary touches itself cannot be equilibrated",
                  tf.index, m.node_ncells[tf.index], m.node_nfcts[tf.index], m.node_nbnd[tf.index]);
  if (tf.verdict == TOPO_BOUNDARY_FACET_UNTYPED)
    return refuse(p, EQLB_ERR_INVALID_ARGUMENT,
                  "eqlb_se_set_boundary: boundary facet %d (nodes %d, %d) has type 0 on right-hand side %d: every "
                  "facet with one cell at an equilibrated node needs a boundary condition",
                  tf.index, m.facet_nodes[2 * (size_t)tf.index], m.facet_nodes[2 * (size_t)tf.index + 1], tf.row);
  if (tf.verdict == TOPO_INTERIOR_FACET_TYPED)
    return refuse(p, EQLB_ERR_INVALID_ARGUMENT,
                  "eqlb_se_set_boundary: facet %d (nodes %d, %d) lies between two cells and has type %d on right-hand "
                  "side %d: only facets with one cell carry boundary conditions",
                  tf.index, m.facet_nodes[2 * (size_t)tf.index], m.facet_nodes[2 * (size_t)tf.index + 1],
                  (int)facet_type[(size_t)tf.row * m.nfacets + tf.index], tf.row);
  return EQLB_OK;
}

// The bin of every equilibrated node, the large patches, and the lane slots and patch indices inside the bins.
// full_first (fused stress launch): the FULL patches of the bins 0, 1 are listed first in their bin - that launch takes
// them, the generic kernels the patches behind them
inline int bin_patches(const HostTopology& m, const PlanOptions& o, const uint8_t* node_mask, bool full_first,
                       BoundaryPlan& p)
{
  p.node_bin.assign(m.nnodes, -1);
  int64_t count[MAX_BINS] = {0, 0, 0, 0, 0};
  for (int32_t i = 0; i < m.nnodes; ++i)
  {
    if (node_mask && !node_mask[i])
      continue;
    int b = 0;
    while (b < MAX_BINS && BIN_P[b] < m.node_nfcts[i])
      ++b;
    if (b < MAX_BINS && m.node_ncells[i] < LARGE_MIN_CELLS)
    {
      p.node_bin[i] = (int8_t)b;
      ++count[b];
      continue;
    }
    if (!o.large_patches)
      return refuse(p, EQLB_ERR_PATCH_TOO_LARGE, "Patch around node %d has %d cells (limit 63)", i, m.node_ncells[i]);
    // option "large_patches": the patch goes to the multi-wave kernel (a CSR-style SoA of its own); its node stays out
    // of the bins and is, for the tiles, a node that another path equilibrates
    if (o.stress && !o.large_patches_stress)
      return refuse(p, EQLB_ERR_PATCH_TOO_LARGE,
                    "Patch around node %d has %d cells: the stress equilibration (weak symmetry, Korn constants) is "
                    "limited to 63 cells per patch, \"large_patches\" covers flux equilibration only",
                    i, m.node_ncells[i]);
    if (o.mode == 1 && o.k >= 4)
      return refuse(p, EQLB_ERR_PATCH_TOO_LARGE,
                    "Patch around node %d has %d cells: the constrained minimisation at RT_4 is limited to 63 cells per "
                    "patch, \"large_patches\" covers it for RT_1 ... RT_3",
                    i, m.node_ncells[i]);
    p.large_nodes.push_back(i);
  }
  for (int b = 0; b < MAX_BINS; ++b)
  {
    p.bins[b].P = BIN_P[b];
    p.bins[b].npatch = count[b];
    p.bins[b].slot_offset = p.nslots;
    p.bins[b].patch_offset = p.npatch_total;
    p.nslots += count[b] * BIN_P[b];
    p.npatch_total += count[b];
    count[b] = 0;
  }
  p.node_slot.assign(m.nnodes, -1);
  p.node_patch.assign(m.nnodes, -1);
  for (int pass = 0; pass < 2; ++pass)
  {
    for (int32_t i = 0; i < m.nnodes; ++i)
    {
      const int b = p.node_bin[i];
      const bool first = full_first && b < 2 && patch_is_full(m.node_ncells[i], m.node_nfcts[i], b);
      if (b < 0 || first != (pass == 0))
        continue;
      p.node_patch[i] = p.bins[b].patch_offset + count[b];
      p.node_slot[i] = p.bins[b].slot_offset + count[b] * BIN_P[b];
      ++count[b];
    }
    if (pass == 0)
      for (int b = 0; b < MAX_BINS; ++b)
        p.bins[b].nfull = count[b];
  }
  return EQLB_OK;
}

// Large patches: lane slots in CSR form (the cell count of a patch is the difference of its offsets), the cells they
// touch, and per patch the work space of the weak-symmetry kernel - quadratic in its cells (the Schur matrix)
inline int plan_large_patches(const HostTopology& m, const PlanOptions& o, BoundaryPlan& p)
{
  const size_t nl = p.large_nodes.size();
  if (nl == 0)
    return EQLB_OK;
  // a large patch inside a group (its two-cell members never are large): the weak-symmetry kernel of the large
  // patches does not read the rows of other patches
  for (int32_t nd : p.large_nodes)
    if (p.any && p.ws[nd] != 0)
      return refuse(p, EQLB_ERR_UNSUPPORTED,
                    "Patch around node %d has %d cells and is the internal patch of group %d of boundary patches with "
                    "tractions on both stress rows: groups are limited to 63 cells per patch (\"large_patches_stress\")",
                    nd, m.node_ncells[nd], p.group[nd]);
  p.l_off.assign(nl + 1, 0);
  std::vector<uint8_t> is_large(m.nnodes, 0);
  int64_t acc = 0;
  for (size_t q = 0; q < nl; ++q)
  {
    const int32_t nd = p.large_nodes[q];
    is_large[nd] = 1;
    p.l_off[q] = (int32_t)acc;
    acc += m.node_ncells[nd];
    p.l_maxcells = std::max(p.l_maxcells, m.node_ncells[nd]);
    if (acc > 0x7fffff00)
      return refuse(p, EQLB_ERR_UNSUPPORTED, "large-patch SoA exceeds 2^31 lane slots");
  }
  p.l_off[nl] = (int32_t)acc;
  p.l_cells = cells_touching(m.cell_nodes, m.ncells, is_large);
  if (o.stress && o.large_wsym_doubles)
  {
    p.l_wsym_off.assign(nl + 1, 0);
    for (size_t q = 0; q < nl; ++q)
      p.l_wsym_off[q + 1] = p.l_wsym_off[q] + (int64_t)o.large_wsym_doubles(o.k, m.node_ncells[p.large_nodes[q]]);
  }
  return EQLB_OK;
}

// What the tiles list.  Plain flux equilibration up to RT_3: every patch of the bins.  Fused stress launch: patches of
// up to 8 facets (bins 0, 1).  Of those, the ones that are not full (interior with fewer cells than lanes, boundary)
// are on the crossed benchmark meshes the boundary patches only (0.4 %) - the tiles list the full patches and the
// others go with the REST (generic kernels on a side stream next to the fused kernel); on unstructured meshes they are
// most patches - the tiles list every patch of the two bins and the kernel carries both instances of the body
// (t_mixed).  EQLB_STRESS_MIXED_TILES=0/1 forces the choice.
inline void plan_tile_lists(const HostTopology& m, const PlanOptions& o, BoundaryPlan& p)
{
  p.tiles = p.t_stress || (!o.stress && o.k <= 3);
  if (!p.tiles)
    return;
  p.tile_bin = p.node_bin;
  if (!p.t_stress)
    return;
  int64_t nlisted = 0, nnotfull = 0;
  for (int32_t i = 0; i < m.nnodes; ++i)
    if (p.node_bin[i] >= 0 && p.node_bin[i] < 2)
    {
      ++nlisted;
      nnotfull += !patch_is_full(m.node_ncells[i], m.node_nfcts[i], p.node_bin[i]);
    }
  p.t_mixed = nnotfull * 20 > nlisted;
  if (const char* env = getenv("EQLB_STRESS_MIXED_TILES"))
    p.t_mixed = env[0] != '0';
  // the rest and the cells of its compact reduction; with large patches, whose rows go through the slot buffer as
  // well, one reduction over the cells that either of them touches
  std::vector<uint8_t> flag(m.nnodes, 0);
  for (int32_t i = 0; i < m.nnodes; ++i)
  {
    const int b = p.node_bin[i];
    if (b >= 2 || (b >= 0 && !p.t_mixed && !patch_is_full(m.node_ncells[i], m.node_nfcts[i], b)))
    {
      p.tile_bin[i] = -1;
      flag[i] = 1;
      ++p.t_rest;
    }
  }
  if (p.t_rest > 0)
    p.rest_cells = cells_touching(m.cell_nodes, m.ncells, flag);
  if (!p.large_nodes.empty())
  {
    for (int32_t nd : p.large_nodes)
      flag[nd] = 1;
    p.l_rest_cells = cells_touching(m.cell_nodes, m.ncells, flag);
  }
}

// What follows the checks: flags, bins, groups, large patches, what the tiles list
inline int plan_patches(const HostTopology& m, const PlanOptions& o, const int8_t* facet_type,
                        const double* boundary_values, const uint8_t* node_mask, BoundaryPlan& p)
{
  if (boundary_values)
  {
    const size_t nb = (size_t)o.nrhs * m.ncells * o.nrt;
    for (size_t i = 0; i < nb && !p.inhomogeneous; ++i)
      p.inhomogeneous = (boundary_values[i] != 0.0);
  }
  if (o.stress)
    for (size_t i = 0; i < (size_t)2 * m.nfacets && !p.stress_flux_bcs; ++i)
      p.stress_flux_bcs = (facet_type[i] == EQLB_FACET_ESSNT_DUAL);
  // RT_2 stress: the fused tiled launch (k_se_stress_tiled) reads DG_1 data; DG_0 data take the route of stress flux
  // BCs - rows into the slots by the patch kernels of the handle's degree, then the weak-symmetry kernel of that route
  // (launch_se_weaksym with no_flux_bcs = false; it reads no DG data, nor do the Korn kernels)
  p.stress_fused_ok = o.k == 2 && o.deg == 1 && !p.stress_flux_bcs;
  p.t_stress = o.stress && p.stress_fused_ok && o.mode == 0;
  if (const int st = bin_patches(m, o, node_mask, p.t_stress, p))
    return st;
  if (o.stress && o.k == 2 && p.stress_flux_bcs)
    if (const int st = find_stress_groups(m, facet_type, node_mask, p))
      return st;
  if (const int st = plan_large_patches(m, o, p))
    return st;
  plan_tile_lists(m, o, p);
  return EQLB_OK;
}

// The plan of an eqlb_se_set_boundary call: the checks, then the patches; p must be a fresh BoundaryPlan.  EQLB_OK, or
// the code of the refusal with its text in p.message.  boundary_values: [nrhs][ncells * nrt] or nullptr.
// (eqlb_se_set_boundary calls the two halves itself, to take the time of each.)
inline int plan_boundary(const HostTopology& m, const PlanOptions& o, const int8_t* facet_type,
                         const double* boundary_values, const uint8_t* node_mask, BoundaryPlan& p)
{
  if (const int st = check_boundary_table(m, o, facet_type, node_mask, p))
    return st;
  return plan_patches(m, o, facet_type, boundary_values, node_mask, p);
}

} // namespace eqlb
