// The handles behind eqlb_se_t / eqlb_ev_t with the boundary tables they own, and the plan of the tiled SoA that the
// tiler hands to the set-up.  Host code only: included by the translation units behind the C ABI, never by a kernel
// file.
#pragma once

#include "eqlb_mesh_handle.h" // (eqlb_boundary_plan.h, eqlb_host_util.h)

namespace eqlb
{
// The tiled SoA as the host plans it (plan_tiles, eqlb_tiling_host.hip): what eqlb_boundary_setup.hip uploads and what
// it hands to the patch builder in instance mode (BuildArgs::inst_*, cell_tile, cell_pos)
struct TilePlan
{
  int32_t ntiles = 0, tc = 0, nprio = 0;
  int64_t nslots = 0;
  int64_t blocks[EQLB_TB_COUNT] = {};
  std::vector<TileDesc> tiles;
  uvec<int32_t> tile_cells, cell_tile, cell_pos; // [ntiles][tc] owned cells (-1: padding); per cell: tile, position
  uvec<int32_t> inst_node, inst_slot, inst_tile; // per patch instance
};

// What eqlb_se_set_boundary builds, and all of it: a new call or the end of the handle drops it as a whole
struct BoundaryTables
{
  bool boundary_set = false;
  bool stress_flux_bcs = true;      // some facet of stress row 0 / 1 carries a flux BC
  bool flat_swept = false;          // a node of the mask is a vertex of a cell of zero area: its patch is left out, every
                                    // sweep raises the status word
  int64_t npatch_total = 0, nslots = 0;
  Bin bins[MAX_BINS];
  DevBuf<int8_t> facet_type;        // [nrhs][nfacets]
  DevBuf<double> bvals;             // [nrhs][ncells*nrt] global boundary DOFs (nullptr: homogeneous)
  DevBuf<int8_t> node_ws;           // grouped stress patches (stress && k == 2 && groups exist)
  DevBuf<int32_t> node_group;
  DevBuf<int8_t> node_wslevel;      // level of the node's group among overlapping groups
  int ws_levels = 1;                // passes of the weak-symmetry kernel
  DevBuf<int64_t> node_slot;        // [nnodes] first slot of the node's patch or -1
  DevBuf<int64_t> node_patch;       // [nnodes] patch index or -1
  DevBuf<int32_t> slot_cell;
  DevBuf<uint32_t> slot_info;
  DevBuf<uint8_t> pn, pflag;
  DevBuf<double> slots;             // [nrhs][ncells][3][nrt]: allocated and zeroed by the first sweep that needs it
                                    // (the node mask may have changed)
  // tiled SoA (plain SE, EQLB_SCATTER_TILED)
  int32_t ntiles = 0, tile_tc = 0;
  bool t_stress = false;            // the tiles serve the fused stress launch (bins P <= 8 only)
  int64_t t_rest = 0;               // patches left to the generic kernels when t_stress (everything but full patches)
  DevBuf<int32_t> rest_cells;       // cells with a vertex whose patch runs on the generic kernels (compact reduction)
  int64_t nrest_cells = 0;
  int64_t t_nslots = 0, t_npatch = 0;
  DevBuf<TileDesc> t_tiles;
  DevBuf<int32_t> t_tile_cells, t_slot_cell, t_facet_owner;
  DevBuf<uint32_t> t_slot_info;
  DevBuf<uint8_t> t_pn, t_pflag;
  // fused stress launch: the tiles list EVERY patch of the bins 0, 1 (full ones first), not the full ones only - where
  // the others are more than a few per cent of the patches (unstructured meshes); kernel with both instances
  bool t_mixed = false;
  int64_t t_blocks[EQLB_TB_COUNT] = {}; // wave-blocks per bin and body instance of the tiled kernel (eqlb_se_tiling_blocks)
  int32_t t_nprio = 0;              // number of priority tiles (numbered first)
  // patches of more than 63 cells or more than 64 facets (option "large_patches"): a CSR-style SoA of their own,
  // outside the five lanes-per-patch bins; k_se_patch_large writes their rows into the slot buffer
  int64_t l_npatch = 0, l_nslots = 0;
  int32_t l_maxcells = 0;
  DevBuf<int32_t> l_off;            // [l_npatch + 1] first lane slot of the patch
  DevBuf<int32_t> l_slot_cell;      // [l_nslots]
  DevBuf<uint32_t> l_slot_info;     // [l_nslots]
  DevBuf<uint8_t> l_pflag;          // [nrhs][l_npatch]
  DevBuf<int32_t> l_cells;          // cells with a vertex whose patch is a large one (compact reduction)
  int64_t l_ncells = 0;
  DevBuf<double> l_ws;              // work space of k_se_patch_large
  bool l_stress = false;            // value of the option "large_patches_stress" when the tables were built
  DevBuf<int32_t> l_nodes;          // [l_npatch] patch nodes (Korn constants)
  DevBuf<int64_t> l_wsym_off;       // [l_npatch] first double of the patch in l_wsym_ws (stress handles)
  DevBuf<double> l_wsym_ws;         // work space of k_se_weaksym_large
  DevBuf<int32_t> l_rest_cells;     // fused stress launch: rest_cells and l_cells merged (one compact reduction)
  int64_t l_nrest_cells = 0;
};

// host side of the tiling (eqlb_tiling_host.hip): tile size, bisection of the cells (cached per mesh), priority order,
// the patch lists of the tiles from bp.tile_bin.  Reads the handle's options and priority cells, writes tp only
int plan_tiles(const eqlb_se* h, const BoundaryPlan& bp, TilePlan& tp);
} // namespace eqlb

struct eqlb_se
{
  eqlb_mesh* mesh = nullptr;
  int k = 0, deg = 0, nrhs = 0, stress = 0;
  int nrt = 0, nd = 0;
  int solver = EQLB_SOLVER_SHUFFLE, scatter = EQLB_SCATTER_AUTO, timing = 0, fused = 1;
  int accumulate = 1;               // option "accumulate": 0 stores the result instead of adding it
  int multi_rhs = 1;                // option "multi_rhs": all right-hand sides of a tiled call in one launch
  int scatter_last = EQLB_SCATTER_SLOTS; // scatter mode the last equilibrate call resolved to
  int mode = 0;                     // 1: constrained-minimisation (EV) patch problems
  int ev_output = 0;                // EV: 0 conforming DOFs, 1 broken hierarchic RT_k layout
  int tile_cells_user = 0;          // option "tile_cells": cells per tile of the tiled launch (0 = automatic)
  int ev_bv_hier = 0;               // EV: boundary values in the hierarchic basis although a basis transform is set
  eqlb::DevBuf<int32_t> ev_cell_dofs; // EV: device copy of the caller's dofmap or nullptr (default)
  int64_t ev_ndofs = 0;             // EV: number of conforming flux DOFs
  eqlb::DevBuf<double> ev_basis;    // EV: device copy of [C (nrt x nrt) | R (k x k) | facet maps 3 x 2 x k x k] or nullptr
  bool ev_basis_has_R = false;
  eqlb::BoundaryTables bt;          // what eqlb_se_set_boundary builds
  // device
  eqlb::DevBuf<double> tables;
  // the side lane of the fused stress launch: the rest's patch kernels run on its stream, next to the fused kernel,
  // between the two events.  Empty until a sweep needs it; built as a whole (eqlb_sweep.hip) or not at all
  struct SideLane
  {
    eqlb::DevStream stream;
    eqlb::DevEvent fork, join;
  } side;
  // two-phase sweeps (multi-GPU overlap): tiles owning a priority cell are numbered first (BoundaryTables::t_nprio)
  std::vector<int32_t> prio_cells;
  int32_t tile_first = 0, tile_count = -1; // options "tile_first" / "tile_count" (-1: to the end)
  int large_patches = 0;            // option "large_patches": patches of more than 63 cells or 64 facets (BoundaryTables::l_*)
  // option "large_patches_stress": weak symmetry and Korn constants on the large patches as well
  int large_patches_stress = 0;
  int slots_first_bin = 0;          // the slot rows of the bins >= this one hold values of the last slot-path run
  eqlb::DevBuf<int32_t> status;
  // staging for host-memory calls: allocated by the first one, kept for the next
  eqlb::DevBuf<double> d_flux_dg, d_rhs_dg, d_flux_hdiv;
  eqlb::DevBuf<double> d_cks, d_korn; // Korn estimate: per node / staging per cell
  // timing ("timing" option): ring of event sets, one set per equilibrate call.  A set holds a begin and an end event
  // per timing slot; the slots are the `which` of eqlb_se_last_kernel_ms
  enum EvSlot
  {
    EV_BIN0 = 0,                // patch kernel of bin b: EV_BIN0 + b (a launch of all bins at once: EV_BIN0)
    EV_REDUCE = eqlb::MAX_BINS, // slot reduction
    EV_WEAKSYM,                 // weak-symmetry kernels
    EV_LARGE,                   // large-patch kernel
    EV_NSLOTS
  };
  static constexpr int ev_begin(int slot) { return 2 * slot; }
  static constexpr int ev_end(int slot) { return 2 * slot + 1; }
  static constexpr int EV_RING = 64, EV_PER_SET = 2 * EV_NSLOTS;
  std::vector<eqlb::DevEvent> ev; // [EV_RING][EV_PER_SET], empty until the first timed call: all of them or none
  int64_t ev_calls = 0;           // calls recorded since timing was (re)enabled
};

struct eqlb_ev
{
  std::unique_ptr<eqlb_se> se; // patch topology, tables, slots, timing of the shared machinery
};
