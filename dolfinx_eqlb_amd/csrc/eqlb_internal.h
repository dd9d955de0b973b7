// Internal structures shared by the host API and the HIP kernels of libeqlb_amd.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/eqlb.h"
#include "eqlb_tuning.h"
#include "eqlb_bins.h" // MAX_BINS, BIN_P, Bin, WS_MAX_LEVELS: shared with the planner of the set-up

namespace eqlb
{

// Packed per-(patch, cell) descriptor, one uint32 per lane slot (lane-contiguous SoA):
//   bits 0-1 fm  local id of E_{a-1} on T_a      bits 2-3 fp  local id of E_a on T_a
//   bits 4-5 ln  local id of the patch node      bit 6 rev_m  E_{a-1} reversed w.r.t. T_{a-1}
//   bit 7 rev_p  E_a reversed w.r.t. T_{a+1}
constexpr uint32_t INFO_FM_SHIFT = 0, INFO_FP_SHIFT = 2, INFO_LN_SHIFT = 4;
constexpr uint32_t INFO_REV_M = 1u << 6, INFO_REV_P = 1u << 7;
//   bits 8-31 (tiled SoA only): 1 + position of the cell among the cells owned by the lane's
//   tile, 0 if the cell belongs to another tile (halo lane: computed, not accumulated)
constexpr uint32_t INFO_LOCAL_SHIFT = 8;

// per-(rhs, patch) flags
constexpr uint8_t PFLAG_INTERIOR = 1, PFLAG_BC0 = 2, PFLAG_BCN = 4;
// grouped boundary patches of the stress path (se/reconstruction.hpp:170-234), in the flags of RHS 0:
// WS_SKIP: two-cell patch of a group, no weak-symmetry step of its own; WS_GROUP: internal patch of a
// group, its weak-symmetry step works on own rows + rows of the group's two-cell patches
constexpr uint8_t PFLAG_WS_SKIP = 8, PFLAG_WS_GROUP = 16;
// level of the patch's group among overlapping groups (bits 5, 6 of the flag of RHS 0): the weak-symmetry kernel
// runs once per level, se/reconstruction.hpp:170-234 treats the groups one after the other
constexpr uint8_t PFLAG_WS_LEVEL_SHIFT = 5;
// slot_info bits 8-10 (plain SoA): local vertex v of the cell belongs to a two-cell patch of the
// lane's group -> its slot row is added to the stress coefficients (bit 8 + v)
constexpr uint32_t INFO_GROUPROW_SHIFT = 8;

// The device arrays of a mesh as every launcher takes them: a plain view that owns nothing.  The owner is the handle
// (struct eqlb_mesh, eqlb_mesh_handle.h), which fills the view from its buffers and keeps the host copies the planners
// read (HostMesh).
struct DeviceMesh
{
  int32_t nnodes = 0, ncells = 0, nfacets = 0, ncells_max = 0;
  const double* x = nullptr;      // [nnodes][3]
  double* cellJ = nullptr;        // [ncells][4] J00 J01 J10 J11 (dx_i/dX_j), cached affine maps (launch_cell_geometry)
  const int32_t *cell_nodes = nullptr, *cell_facets = nullptr, *facet_nodes = nullptr;
  const int32_t *facet_cells_off = nullptr, *facet_cells = nullptr;
  const int32_t *node_cells_off = nullptr, *node_facets_off = nullptr, *node_facets = nullptr;
  const int32_t* node_cells = nullptr; // nullptr until mesh_node_cells() of the handle has uploaded it: read it there
  const uint8_t* facet_perm = nullptr;
};

// kernel arguments of the patch kernel (one launch per bin)
struct SeArgs
{
  const double* cellJ;
  const int32_t* slot_cell;   // [nslots] global cell id or -1
  const uint32_t* slot_info;  // [nslots]
  const uint8_t* pn;          // [npatch] cells per patch
  const uint8_t* pflag;       // [nrhs][npatch_total]
  const double* tables;       // S | F | H | D
  const double* flux_dg;      // [nrhs][ncells*ND*2]
  const double* rhs_dg;       // [nrhs][ncells*ND]
  const double* bvals;        // [nrhs][ncells*NRT] global flux-boundary DOFs or nullptr (homogeneous)
  double* out;                // slots [nrhs][ncells][3][NRT] or flux_hdiv [nrhs][ncells*NRT]
  int32_t* status;            // device error flag
  int64_t npatch;             // patches of this bin
  int64_t slot_offset, patch_offset, npatch_total;
  int32_t ncells, nrhs;
  int32_t rhs;                // index of the right-hand side handled by this launch (flags, bvals)
  int32_t rhs_in, rhs_out;    // block index of that right-hand side inside flux_dg / rhs_dg and inside out
                              // (0 when the pointers already address the block: lists of separate arrays)
  int32_t ws_level = 0;       // weak-symmetry kernels: the pass handles the patches of this group level
};

// bins of a fused launch: blocks [block_start[b], block_start[b+1]) of 256 threads handle bin b
struct FusedBins
{
  int64_t block_start[MAX_BINS + 1];
  int64_t npatch[MAX_BINS], slot_offset[MAX_BINS], patch_offset[MAX_BINS];
};

// Tiled launch (EQLB_SCATTER_TILED): a workgroup owns TC cells (a leaf of the recursive coordinate
// bisection of the cell centroids), solves every patch that touches one of them and accumulates the
// three vertex contributions of its cells in LDS, so neither the slot buffer nor the reduction pass
// exist.
struct TileDesc
{
  int32_t slot_start[MAX_BINS]; // first lane slot of the tile's patches of bin b (multiple of 64)
  int32_t patch_start[MAX_BINS];
  int32_t npatch[MAX_BINS];
  int32_t nfull[MAX_BINS]; // leading patches of the bin that are interior with exactly P cells
  int32_t nint[MAX_BINS];  // leading patches that are interior (no boundary facet), nfull of them full
  // behind the full ones the interior patches are ordered by their number of cells: nval[b][j] = end (in patches of the
  // bin) of those with P - 1 - j cells, j = 0, 1, 2; the other interior patches follow up to nint (bins 0, 1 only)
  int32_t nval[2][3];
  int32_t zero;            // 1: a vertex of an owned cell is not equilibrated here (node mask): its row
                           // is never written, the LDS slots of the tile are zeroed first
};

// Wave-block ranges of one bin of a tile's patch list (P lanes per patch, 64 / P patches per wave-block). The tiled
// kernels (k_se_patch_tiled*, k_se_stress_tiled) split their lists with these functions, and so does the host count
// behind eqlb_se_tiling_blocks: it reports what the kernels run.
// k_se_patch_tiled: an instance for whole wave-blocks of full patches (RT_1: the body is too small for the second
// instance to pay), and one for whole wave-blocks of interior patches of any size (K = 2, P = 8, 16; for RT_3, P = 8
// as well: no gain on the Delaunay mesh, 0.413 - 0.418 ms either way)
__host__ __device__ constexpr bool tile_spec_full(int K, int P) { return P <= 8 && K >= 2; }
__host__ __device__ constexpr bool tile_spec_interior(int K, int P) { return K == 2 && (P == 8 || P == 16); }
// wave-blocks of the first n patches: all of them (the last one may be partly empty) / the whole ones only
__host__ __device__ __forceinline__ int tile_wb_all(int n, int P) { return (n * P + 63) >> 6; }
__host__ __device__ __forceinline__ int tile_wb_whole(int n, int P) { return (n * P) >> 6; }
// k_se_stress_tiled with mixed lists: the whole wave-blocks [c0, c1) of the interior patches with P - 1 - j cells,
// j = 0, 1, 2 (the patches nval[B][j - 1] ... nval[B][j] of the bin; from nfull[B] for j = 0); c1 = c0 where no whole
// block lies inside, or where that instance does not exist (P - 1 - j < 3)
template <int P>
__host__ __device__ __forceinline__ void tile_nfix_range(const TileDesc& td, int B, int j, int& c0, int& c1)
{
  constexpr int PER = 64 / P;
  const int first = (j == 0) ? td.nfull[B] : td.nval[B][j - 1];
  c0 = (first + PER - 1) / PER;
  c1 = (P - 1 - j >= 3) ? td.nval[B][j] / PER : 0;
  if (c1 < c0)
    c1 = c0;
}

struct TileArgs
{
  const TileDesc* tiles;
  const int32_t* tile_cells; // [ntiles][tc] owned cells (-1: padding)
  int32_t ntiles, tc;
  // EV flush to the conforming DOFs (nullptr: broken layout)
  const int32_t* facet_owner; // [ntiles][tc][3] 2 * facet + reversal bit, or -1
  const int32_t* cell_dofs;   // caller's dofmap or nullptr (default numbering)
  int64_t ndofs;
  int32_t nfacets;
  int32_t tile_first; // this launch handles the tiles [tile_first, tile_first + ntiles)
  int32_t accumulate; // 1: flux_hdiv += result (reference semantics), 0: flux_hdiv = result (no read of the old values)
  // EV: change of basis of the conforming output (eqlb_ev_set_basis_transform) or nullptr (hierarchic RT_k):
  // target cell DOFs = basis_C x broken hierarchic cell DOFs; basis_R: facet block of a reversed facet
  const double* basis_C;
  const double* basis_R;
};

// right-hand sides of a multi-RHS tiled launch (k_se_patch_tiled_multi)
constexpr int MULTI_RHS_MAX = 8;
struct MultiRhs
{
  int32_t n, rhs0; // right-hand sides rhs0 .. rhs0 + n - 1 of the handle (boundary flags, boundary values)
  const double* g[MULTI_RHS_MAX];
  const double* f[MULTI_RHS_MAX];
  double* x[MULTI_RHS_MAX];
};

struct BuildArgs
{
  int32_t nnodes, nfacets, nrhs;
  const int32_t *cell_nodes, *cell_facets, *facet_nodes, *facet_cells_off, *facet_cells;
  const int32_t *node_cells_off, *node_facets_off, *node_facets;
  const uint8_t* facet_perm;
  const int8_t* facet_type;  // [nrhs][nfacets]
  const int64_t* node_slot;  // first lane slot of the node's patch, -1: not equilibrated
  const int64_t* node_patch; // patch index
  int64_t npatch_total;
  int32_t* slot_cell;
  uint32_t* slot_info;
  uint8_t* pn;
  uint8_t* pflag;
  // grouped stress patches (nullptr: none): per node 0 / 1 (two-cell member) / 2 (internal patch of
  // a group) and the group id
  const int8_t* node_ws;
  const int32_t* node_group;
  const int8_t* node_wslevel;
  // instance mode (tiled SoA): thread i builds the patch of node inst_node[i] at slot inst_slot[i]
  // as patch i of tile inst_tile[i]; nullptr: one patch per node (node_slot / node_patch)
  int64_t ninst;
  const int32_t* inst_node;
  const int32_t* inst_slot;
  const int32_t* inst_tile;
  const int32_t* cell_tile; // [ncells] owning tile
  const int32_t* cell_pos;  // [ncells] position in the tile-sorted cell list
  int32_t tile_cells;       // cells per tile
  // optional export in OrientedPatch layout (nullptr: off)
  int32_t stride;
  int32_t *ex_ncells, *ex_cells, *ex_fcts;
  int8_t *ex_fl, *ex_il, *ex_rev;
  // 1: fans of any length are walked (large-patch SoA, export of a handle with "large_patches"); pn may then be
  // nullptr (the CSR offsets of that SoA hold the cell counts, a uint8_t would wrap at 256)
  int32_t large;
};

void launch_build_patches(const BuildArgs& a, hipStream_t stream);
void launch_cell_geometry(int32_t ncells, const double* x, const int32_t* cell_nodes,
                          double* cellJ, hipStream_t stream);
// cells whose det J is zero to rounding or not finite: node_flat [nnodes] (zeroed by the caller) gets 1 at their three
// vertices, *count their number
void launch_flat_cell_nodes(int32_t ncells, const double* cellJ, const int32_t* cell_nodes, uint8_t* node_flat,
                            int32_t* count, hipStream_t stream);
// returns 0 or EQLB_ERR_UNSUPPORTED
int launch_se_patch(int k, int deg, int P, int solver, int scatter, const SeArgs& a,
                    hipStream_t stream, int mode = 0);
int launch_se_patch_fused(int k, int deg, int scatter, const SeArgs& a, const FusedBins& fb,
                          hipStream_t stream);
int launch_se_patch_tiled(int k, int deg, int mode, const SeArgs& a, const TileArgs& t, hipStream_t stream);
int launch_se_patch_tiled_multi(int k, int deg, int mode, const SeArgs& a, const TileArgs& t, const MultiRhs& mr,
                                hipStream_t stream);
// RT_2 / P1, SE mode: the tiled launch whose full 8-cell patches run on four lanes, two ring cells per lane
// (eqlb_se_kernels_pair.hip); launch_se_patch_tiled hands over to it where the instance is built and the handle has
// one right-hand side
bool pair_lanes_built();
int launch_se_patch_tiled_pair(const SeArgs& a, const TileArgs& t, hipStream_t stream);
// the same launches for projected data of degree deg < k - 1 (eqlb_se_kernels_lowdeg*.hip): the launchers above hand
// every call with deg != k - 1 over to these
int launch_se_patch_lowdeg(int k, int deg, int P, int solver, int scatter, const SeArgs& a, hipStream_t stream,
                           int mode);
int launch_se_patch_fused_lowdeg(int k, int deg, int scatter, const SeArgs& a, const FusedBins& fb,
                                 hipStream_t stream);
int launch_se_patch_tiled_lowdeg(int k, int deg, int mode, const SeArgs& a, const TileArgs& t, hipStream_t stream);
int launch_se_patch_tiled_multi_lowdeg(int k, int deg, int mode, const SeArgs& a, const TileArgs& t,
                                       const MultiRhs& mr, hipStream_t stream);
int launch_ev_patch_fused_lowdeg(int k, int deg, const SeArgs& a, const FusedBins& fb, hipStream_t stream);
int launch_se_patch_k4_lowdeg(int deg, int P, int solver, int scatter, const SeArgs& a, hipStream_t stream,
                              int mode); // eqlb_se_kernels_lowdeg_k4.hip
int fill_tables_k4_lowdeg(int deg, std::vector<double>& out); // tables of RT_4 / DG_deg, deg < 3
void launch_tile_facet_owner(const DeviceMesh& m, int64_t n, const int32_t* tile_cells, int32_t* code,
                             hipStream_t stream);
int tile_cells_of(int k);
int tile_cells_ev_of(int k);
int tile_cells_max_of(int k);
// patches of more than 63 cells / 64 facets, one workgroup per patch (eqlb_se_large.hip): a.slot_cell / slot_info /
// pflag / npatch_total address the large-patch SoA, off its CSR offsets [npatch + 1], a.out the slot buffer;
// ws: large_patch_ws_doubles(k, lane slots, patches) doubles of work space
int launch_se_patch_large(int k, int deg, int mode, const SeArgs& a, const int32_t* off, double* ws,
                          hipStream_t stream);
size_t large_patch_ws_doubles(int k, int64_t nslots, int64_t npatch);
// weak symmetry of the stress rows 0, 1 on the large patches (eqlb_se_weaksym_large.hip, RT_2 ... RT_4): a addresses the
// large-patch SoA as for launch_se_patch_large, a.out the slot buffer that holds the rows of that kernel; patch p works in
// ws + wsoff[p], large_patch_weaksym_ws_doubles(k, cells of the patch) doubles (quadratic in the cells: the Schur matrix)
int launch_se_weaksym_large(int k, const SeArgs& a, const int32_t* off, const int64_t* wsoff, double* ws,
                            hipStream_t stream);
size_t large_patch_weaksym_ws_doubles(int k, int64_t ncells_of_patch);
int launch_se_weaksym(int k, int P, bool no_flux_bcs, const SeArgs& a, hipStream_t stream);
// RT_4 with P >= 16 and RT_3 with P = 64 (banded chain + border, eqlb_se_weaksym_banded.hip)
int launch_se_weaksym_banded(int k, int P, const SeArgs& a, hipStream_t stream);
// fused stress launch (RT_2, no stress flux BCs, patches of up to 8 facets): rows 0, 1 + weak symmetry
// mixed: tile lists with every patch of up to 8 lanes (full ones first; generic instance of the body for the others),
// else lists of full patches only
int launch_se_stress_tiled(const SeArgs& a, const TileArgs& t, const double* const* g, const double* const* f,
                           double* const* x, hipStream_t stream, bool mixed = false);
int stress_tile_cells();
int launch_ev_patch_fused(int k, int deg, const SeArgs& a, const FusedBins& fb, hipStream_t stream);
// conforming <-> broken layout of the EV equilibrator (eqlb_ev.hip); cell_dofs may be nullptr
// (default numbering: facet*k + j, then nfacets*k + cell*(k^2-k) + i)
// facet_maps: nullptr (hierarchic RT_k: -I / B) or [3][2][k][k]: broken facet DOFs = map[lf][reversed] x conforming ones
void launch_ev_boundary_to_broken(const DeviceMesh& m, int k, int nrhs, const int32_t* cell_dofs,
                                  int64_t ndofs, const double* bv_conf, double* bv_broken,
                                  const double* facet_maps, hipStream_t stream);
void launch_ev_reduce(const DeviceMesh& m, int k, int nrhs, const int32_t* cell_dofs, int64_t ndofs,
                      const double* slots, double* x, int accumulate, const double* basis_C, const double* basis_R,
                      hipStream_t stream);
int launch_reduce_slots(int nrt, int32_t ncells, int32_t nrhs, const double* slots, double* x, int accumulate,
                        hipStream_t stream);
int launch_reduce_slots_cells(int nrt, int32_t ncells, int64_t nlist, const int32_t* cells, const double* slots,
                              double* x, hipStream_t stream);
int projection_matrix_host(int degree, int nq, const double* pts, const double* wts,
                           std::vector<double>& Pm);
void launch_project_dg(int64_t ncells, int nd, int nq, int bs, const double* Pm, const double* qv,
                       double* out, hipStream_t stream);
// l_npatch > 0: the fans of the large patches as well, through their SoA (l_nodes: the patch nodes)
void launch_korn(const DeviceMesh& m, const int64_t* node_slot, const int64_t* node_patch,
                 const int32_t* slot_cell, const uint32_t* slot_info, const uint8_t* pn,
                 const uint8_t* pflag, double* cks, double* korn, hipStream_t stream, int64_t l_npatch = 0,
                 const int32_t* l_nodes = nullptr, const int32_t* l_off = nullptr, const int32_t* l_slot_cell = nullptr,
                 const uint32_t* l_slot_info = nullptr, const uint8_t* l_pflag = nullptr);
// the weight of eqlb_se_estimate_weighted / eqlb_ev_estimate_weighted: W_T = adj(D_T) / (kappa_T det D_T) with
// kappa_T = cell_coeff[cell] and D_T = (d00, d01, d11) = cell_D[cell] where given, else 1 and the identity.  A kernel
// argument of the weighted variant, which the kernels of the entries without a weight do not take
struct EstWeightArgs
{
  const double* cell_coeff = nullptr; // [ncells] or nullptr
  const double* cell_D = nullptr;     // [ncells][3] or nullptr
};
// estimator step (eqlb_estimate.hip); flux_dg / rhs_dg in DG_deg, 0 <= deg <= k - 1.  wx == nullptr: the kernels without
// a weight; else sig2 is the weighted flux norm
int launch_estimate(const DeviceMesh& m, int k, int deg, int nrhs, const double* x_eq, const double* flux_dg,
                    const double* rhs_dg, double* div2, double* sig2, double* jump, double alpha,
                    double beta, hipStream_t stream, const EstWeightArgs* wx = nullptr);
int launch_boundary_residual(const DeviceMesh& m, int k, int deg, int nrhs, const double* x_eq,
                             const double* flux_dg, int32_t nlist, const int32_t* facets, const double* bvals,
                             double* out, hipStream_t stream);
// the cell-wise coefficients of eqlb_se_estimate_stress_mu: pi_T = cell_pi1[cell] and mu_T = cell_mu[cell] where given,
// else the scalars.  A kernel argument of the variant with them, which the kernel of eqlb_se_estimate_stress does not take
struct StressCoeffArgs
{
  const double* cell_pi1 = nullptr; // [ncells] or nullptr
  const double* cell_mu = nullptr;  // [ncells] or nullptr
  double pi_1 = 1.0, mu = 1.0;
};
// co == nullptr: the kernel with the scalar pi_1 and mu = 1
int launch_estimate_stress(const DeviceMesh& m, const int32_t* node_cells, int k, const double* x0,
                           const double* x1, const double* korn, double pi_1, double* energy, double* wsym,
                           double* node_asym, hipStream_t stream, const StressCoeffArgs* co = nullptr);
int launch_oscillation(const DeviceMesh& m, int k, int deg, int nrhs, const double* x_eq, const double* flux_dg,
                       int nq, const double* qpoints, const double* qweights, const double* fvalues,
                       const double* korn, double* out, hipStream_t stream);
// the same launches for deg < k - 1 (eqlb_estimate_lowdeg.hip, which passes k = 4 on to eqlb_estimate_lowdeg_k4.hip):
// the launchers above hand every call with deg != k - 1 over to these
int launch_estimate_lowdeg(const DeviceMesh& m, int k, int deg, int nrhs, const double* x_eq, const double* flux_dg,
                           const double* rhs_dg, double* div2, double* sig2, double* jump, double alpha,
                           double beta, hipStream_t stream, const EstWeightArgs* wx = nullptr);
int launch_boundary_residual_lowdeg(const DeviceMesh& m, int k, int deg, int nrhs, const double* x_eq,
                                    const double* flux_dg, int32_t nlist, const int32_t* facets,
                                    const double* bvals, double* out, hipStream_t stream);
int launch_oscillation_lowdeg(const DeviceMesh& m, int k, int deg, int nrhs, const double* x_eq,
                              const double* flux_dg, int nq, const double* qpoints, const double* qweights,
                              const double* fvalues, const double* korn, double* out, hipStream_t stream);
int launch_estimate_k4_lowdeg(const DeviceMesh& m, int deg, int nrhs, const double* x_eq, const double* flux_dg,
                              const double* rhs_dg, double* div2, double* sig2, double* jump, double alpha,
                              double beta, hipStream_t stream, const EstWeightArgs* wx = nullptr);
int launch_boundary_residual_k4_lowdeg(const DeviceMesh& m, int deg, int nrhs, const double* x_eq,
                                       const double* flux_dg, int32_t nlist, const int32_t* facets,
                                       const double* bvals, double* out, hipStream_t stream);
int launch_oscillation_k4_lowdeg(const DeviceMesh& m, int deg, int nrhs, const double* x_eq, const double* flux_dg,
                                 int nq, const double* qpoints, const double* qweights, const double* fvalues,
                                 const double* korn, double* out, hipStream_t stream);
int set_error(int code, const char* fmt, ...); // thread-local message of eqlb_last_error + the code back
void launch_halo_pack(int nrhs, int32_t nlist, int32_t nrt, int64_t ncells, const int64_t* cells, double* x,
                      double* buf, int clear, hipStream_t stream);
void launch_halo_unpack_add(int nrhs, int32_t nlist, int32_t nrt, int64_t ncells, const int64_t* cells,
                            double* x, const double* buf, hipStream_t stream);
// tiles by recursive coordinate bisection on the device (eqlb_tiling_device.hip): 0 ok, 1 stretched mesh (host
// bisection), < 0 device error
void device_tiling_prepare();
int device_tile_order(const DeviceMesh& m, int tc, int32_t ntiles, const double blo[2], const double bhi[2], double inv,
                      std::vector<int32_t>& order);
size_t table_doubles(int k, int deg);
size_t table_offset_te(int k, int deg); // first double of TE in the table buffer (Sizes::OFF_TE)
int fill_tables_host(int k, int deg, std::vector<double>& out);

} // namespace eqlb

struct eqlb_mesh; // the handle behind eqlb_mesh_t: eqlb_mesh_handle.h (host code only)
struct eqlb_refine; // the plan behind eqlb_refine_t: eqlb_refine_plan.h (host code only)
struct eqlb_primal; // the solver handles: eqlb_primal_solve.hip, eqlb_primal_elasticity.hip
struct eqlb_elasticity;

namespace eqlb
{
// ---- the columns of a P_p solve: 1 ... MANY_R right-hand sides in one launch (eqlb_primal_common.h states the rule) ----
constexpr int MANY_R = 4; // columns of one group; more run group after group

// scalars of the iteration of one column, in device memory
struct PcgState
{
  double rho, pq, alpha, beta, rr, nb, tol, rtrue;
  int32_t iters, done, breakdown, converged, replacements, pad;
};

// The columns a launch works on: R <= MANY_R columns lie one after another (vectors [R][n], y_loc [R][ncells nd_p bs],
// block partials [R][2][G], states [R]).  Column c runs if bit c of mask is set and, with check, the stop flag of its
// state st[c] is not set; the others are neither read nor written.  A launch that knows no state: check = 0, st = nullptr
struct ManyCols
{
  int32_t R;
  uint32_t mask;
  int32_t check;
  const PcgState* st; // [R] DEVICE
};

// bit c: column c runs in this launch; NC: the column slots of the kernel (R <= NC)
template <int NC>
__device__ __forceinline__ uint32_t cols_live(const ManyCols& c)
{
  uint32_t live = 0;
#pragma unroll
  for (int k = 0; k < NC; ++k)
    if (k < c.R && ((c.mask >> k) & 1u) && !(c.check && c.st[k].done))
      live |= 1u << k;
  return live;
}
// column k of a kernel with NC slots runs (behind `if (!live) return;` the one column of NC = 1 does)
template <int NC>
__device__ __forceinline__ bool col_on(uint32_t live, int k)
{
  return NC == 1 || ((live >> k) & 1u);
}

// The work space of a solver handle for R columns of n rows each, all DEVICE: a view that owns nothing.  One column is
// carved out of the handle's allocation at create; more (Poisson handles only) are grown by the first call that needs
// them and reused afterwards
struct PcgWork
{
  int64_t n; // rows of a column: bs * ndofs
  int R;     // columns of the launches on it
  const double* diag;
  const uint8_t* fixed;
  double *yloc, *r, *z, *d, *q, *part; // y_loc [R][ncells nd_p bs], vectors [R][n], block partials [R][2][G]
  PcgState* st;                        // [R]
};

// A solver handle (eqlb_primal_t, bs = 1; eqlb_elasticity_t, bs = 2) as the hierarchy unit eqlb_multilevel.hip sees it:
// a view that owns nothing.  All pointers DEVICE; vectors have bs * ndofs rows per column.  The launches are those of
// the handle's own unit, on its own kernels; they work on the columns of c in the work space for c.R columns.
struct SolverLevel
{
  void* handle;
  eqlb_mesh* mesh;
  int p, bs;
  int64_t ndofs;            // scalar count
  const int32_t* cell_dofs; // [ncells][nd_p]
  const double* diag;
  const uint8_t* fixed;
  const int32_t* status;    // [4] the status word of the mask (skipped ids, listed valid ones per component)
  // the work space for R columns (R > 1: grown here if need be; an elasticity handle refuses); to be called before a
  // launch on R columns
  int (*work)(void* handle, int R, PcgWork& w);
  // y = owner sum of y_loc (0 on the fixed rows if masked)
  hipError_t (*owner_sum)(void* handle, const ManyCols& c, double* y, bool masked, hipStream_t stream);
  // r = b - A u (0 on the fixed rows; u^ instead of u with only_fixed), the block partials of r.r in part
  hipError_t (*residual)(void* handle, const ManyCols& c, const double* b, const double* u, double* r, bool only_fixed,
                         hipStream_t stream);
  // q = A d on the free rows, the block partials of d.q in part
  hipError_t (*product)(void* handle, const ManyCols& c, hipStream_t stream);
  // the operator is positive definite without a fixed DOF: a Robin term with some weight > 0 (eqlb_primal_set_robin)
  bool (*definite)(void* handle);
};
void primal_level(eqlb_primal* h, SolverLevel& v);
void elasticity_level(eqlb_elasticity* h, SolverLevel& v);
// eqlb_transfer.hip: the store pass of the restriction r = P^T r2 from `refined` to the mesh of `plan` on the columns
// of c: r2 [R][ndofs2 bs] into yloc [R][ncells nd_p bs] (bs = 2: one column); DEVICE pointers, one launch, nothing waits
int launch_restrict(const char* who, eqlb_refine* plan, eqlb_mesh* refined, int p, int bs, const ManyCols& c,
                    const int32_t* cell_dofs2, int64_t ndofs2, const double* r2, double* yloc, hipStream_t stream);
} // namespace eqlb

struct eqlb_se; // the handle behind eqlb_se_t / eqlb_ev_t: eqlb_handle.h (host code only)
