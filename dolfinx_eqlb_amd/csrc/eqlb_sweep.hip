// The equilibration sweep behind eqlb_se_equilibrate*: resolves the scatter mode of a call, stages host data, and
// issues the launches of the tiled, the slot or the atomic route.  Host code only; the kernels and their launchers
// live in the eqlb_se_*.hip / eqlb_stress_tiled.hip / eqlb_ev.hip files.
#include "eqlb_handle.h"

#include <algorithm>

namespace
{

// What one call works with.  Built once by equilibrate_lists; the steps below read it and change nothing in it.
struct Sweep
{
  eqlb_se* h;
  const eqlb::DeviceMesh& m;
  hipStream_t stream;      // the caller's stream
  int scatter;             // EQLB_SCATTER_SLOTS / _ATOMIC / _TILED (AUTO resolved)
  bool stress_fused;       // stress of RT_2 without flux BCs on the stress rows: rows 0, 1 and their weak symmetry in
                           // one tiled launch
  bool ev_conf;            // EV mode writes conforming DOFs unless the broken layout is requested
  size_t s_g, s_f, s_slot, s_x; // doubles per right-hand side: flux_dg, rhs_dg, broken RT coefficients, output
  const double* const* d_g;     // device blocks of the right-hand sides
  const double* const* d_f;
  double* const* d_x;
  eqlb::SeArgs a;          // arguments common to the patch kernels of the call
  const eqlb::DevEvent* evs; // event set of this call, or nullptr (option "timing" off)
};

// Resolves EQLB_SCATTER_AUTO - the tiled launch where it applies and is the fastest (k <= 3, plain flux
// equilibration, shuffle solver), else slots + reduction - and refuses what the resolved route
// does not offer.  h->scatter_last holds the resolved mode also where the call is refused.
int plan_sweep(eqlb_se* h, int& scatter, bool& stress_fused)
{
  scatter = h->scatter;
  stress_fused = h->stress && h->bt.t_stress && h->bt.ntiles > 0 && h->solver == EQLB_SOLVER_SHUFFLE
                 && (scatter == EQLB_SCATTER_AUTO || scatter == EQLB_SCATTER_TILED);
  if (scatter == EQLB_SCATTER_AUTO)
    scatter = (stress_fused || (!h->stress && h->k <= 3 && h->solver == EQLB_SOLVER_SHUFFLE && h->bt.ntiles > 0))
                  ? EQLB_SCATTER_TILED
                  : EQLB_SCATTER_SLOTS;
  h->scatter_last = scatter;
  if (!h->accumulate && scatter == EQLB_SCATTER_ATOMIC)
    return fail(EQLB_ERR_UNSUPPORTED, "\"accumulate\" = 0 is not available with the atomic scatter");
  if (h->bt.l_npatch > 0 && scatter == EQLB_SCATTER_ATOMIC)
    return fail(EQLB_ERR_UNSUPPORTED,
                "patches of more than 63 cells (\"large_patches\") run with the slot or the tiled scatter, not the atomic one");
  if (h->mode == 1 && (scatter == EQLB_SCATTER_ATOMIC || (h->solver != EQLB_SOLVER_SHUFFLE && h->k != 4)))
    return fail(EQLB_ERR_UNSUPPORTED, "EV equilibration runs with the shuffle solver (tiled or slot scatter)");
  if (scatter == EQLB_SCATTER_TILED)
  {
    if ((h->stress && !stress_fused) || h->solver != EQLB_SOLVER_SHUFFLE || h->bt.ntiles == 0)
      return fail(EQLB_ERR_UNSUPPORTED,
                  "the tiled scatter is available for k <= 3 with the shuffle solver (stress: RT_2 without "
                  "flux boundary conditions on the stress rows)");
    if (h->tile_first > h->bt.ntiles)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "tile_first %d beyond the %d tiles", h->tile_first, h->bt.ntiles);
  }
  if (scatter == EQLB_SCATTER_ATOMIC && h->stress)
    return fail(EQLB_ERR_UNSUPPORTED, "stress equilibration needs the slot or the tiled scatter");
  return EQLB_OK;
}

// Host-memory calls: the caller's blocks go through the staging buffers of the handle
int stage_in(eqlb_se* h, size_t s_g, size_t s_f, size_t s_x, const double* const* g_in, const double* const* f_in,
             double* const* x_io, const double** d_g, const double** d_f, double** d_x, hipStream_t stream)
{
  if (!h->d_flux_dg)
  {
    if (h->d_flux_dg.alloc(h->nrhs * s_g) || h->d_rhs_dg.alloc(h->nrhs * s_f) || h->d_flux_hdiv.alloc(h->nrhs * s_x))
      return EQLB_ERR_DEVICE;
  }
  for (int r = 0; r < h->nrhs; ++r)
  {
    HIP_TRY(hipMemcpyAsync(h->d_flux_dg + r * s_g, g_in[r], s_g * sizeof(double), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(h->d_rhs_dg + r * s_f, f_in[r], s_f * sizeof(double), hipMemcpyHostToDevice, stream));
    if (h->accumulate)
      HIP_TRY(hipMemcpyAsync(h->d_flux_hdiv + r * s_x, x_io[r], s_x * sizeof(double), hipMemcpyHostToDevice, stream));
    d_g[r] = h->d_flux_dg + r * s_g;
    d_f[r] = h->d_rhs_dg + r * s_f;
    d_x[r] = h->d_flux_hdiv + r * s_x;
  }
  return EQLB_OK;
}

// ... and back; the host caller also learns of a patch system that was not positive definite
int stage_out(eqlb_se* h, size_t s_x, double* const* x_io, double* const* d_x, hipStream_t stream)
{
  for (int r = 0; r < h->nrhs; ++r)
    HIP_TRY(hipMemcpyAsync(x_io[r], d_x[r], s_x * sizeof(double), hipMemcpyDeviceToHost, stream));
  int32_t status = 0;
  HIP_TRY(hipMemcpyAsync(&status, h->status, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  if (status)
  {
    HIP_TRY(hipMemsetAsync(h->status, 0, sizeof(int32_t), stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return fail(EQLB_ERR_SINGULAR, "patch system not positive definite");
  }
  return EQLB_OK;
}

// Option "timing": the event set of this call in the ring of the handle (created on first use)
int timing_events(eqlb_se* h, const eqlb::DevEvent*& evs)
{
  if (h->ev.empty())
  {
    std::vector<eqlb::DevEvent> ring(eqlb_se::EV_RING * eqlb_se::EV_PER_SET);
    for (eqlb::DevEvent& e : ring)
      HIP_TRY(e.create(hipEventDefault));
    h->ev = std::move(ring);
  }
  evs = h->ev.data() + (h->ev_calls % eqlb_se::EV_RING) * eqlb_se::EV_PER_SET;
  return EQLB_OK;
}

// begin / end of a timing slot on a stream; evs == nullptr: untimed
int mark_begin(const eqlb::DevEvent* evs, int slot, hipStream_t st)
{
  if (evs)
    HIP_TRY(hipEventRecord(evs[eqlb_se::ev_begin(slot)], st));
  return EQLB_OK;
}
int mark_end(const eqlb::DevEvent* evs, int slot, hipStream_t st)
{
  if (evs)
    HIP_TRY(hipEventRecord(evs[eqlb_se::ev_end(slot)], st));
  return EQLB_OK;
}

// data of right-hand side r: the kernels address block rhs_in of flux_dg / rhs_dg and block rhs_out
// of out; the caller's arrays arrive block by block, the slot buffer is one array
void select_rhs(const Sweep& s, eqlb::SeArgs& aa, int r, bool to_slots)
{
  aa.rhs = r;
  aa.flux_dg = s.d_g[r];
  aa.rhs_dg = s.d_f[r];
  aa.rhs_in = 0;
  aa.out = to_slots ? s.h->bt.slots : s.d_x[r];
  aa.rhs_out = to_slots ? r : 0;
}

// change of basis of the conforming EV output: the facet block of a reversed facet lies behind C in ev_basis
const double* basis_R(const eqlb_se* h)
{
  return (h->ev_basis && h->ev_basis_has_R) ? h->ev_basis + h->nrt * h->nrt : nullptr;
}

// Patches of the plain SoA that a group of launches handles: per bin a count and the offsets of the first one
struct PatchRange
{
  int64_t npatch[eqlb::MAX_BINS], slot_offset[eqlb::MAX_BINS], patch_offset[eqlb::MAX_BINS];
};

PatchRange all_patches(const eqlb_se* h)
{
  PatchRange pr;
  for (int b = 0; b < eqlb::MAX_BINS; ++b)
  {
    pr.npatch[b] = h->bt.bins[b].npatch;
    pr.slot_offset[b] = h->bt.bins[b].slot_offset;
    pr.patch_offset[b] = h->bt.bins[b].patch_offset;
  }
  return pr;
}

// The REST of a fused stress launch: in the bins 0, 1 the patches behind the full ones (Bin::nfull) - none of them
// where the tiles list every patch of those bins (t_mixed) -, the higher bins entirely
PatchRange rest_of_fused_stress(const eqlb_se* h)
{
  PatchRange pr = all_patches(h);
  for (int b = 0; b < 2; ++b)
  {
    const eqlb::Bin& bin = h->bt.bins[b];
    pr.npatch[b] = h->bt.t_mixed ? 0 : bin.npatch - bin.nfull;
    pr.slot_offset[b] += bin.nfull * bin.P;
    pr.patch_offset[b] += bin.nfull;
  }
  return pr;
}

// Which rows of the slot buffer the patch kernels of a run rewrite (eqlb_se::slots_first_bin keeps the last one)
enum SlotCover
{
  COVER_ALL = 0,                 // every patch of the bins
  COVER_REST = 1,                // the rest of a fused stress launch
  COVER_LARGE = eqlb::MAX_BINS   // the large patches only
};

// The slot buffer, zeroed where rows of an earlier run that covered more than `cover` would be added again
int ensure_slots(const Sweep& s, SlotCover cover, hipStream_t st)
{
  eqlb_se* h = s.h;
  const size_t bytes = (size_t)h->nrhs * s.s_slot * 3 * sizeof(double);
  if (!h->bt.slots)
  {
    if (h->bt.slots.alloc(bytes / sizeof(double)))
      return EQLB_ERR_DEVICE;
    // slots of (cell, vertex) pairs whose node is not equilibrated here (node_mask, other path) stay zero
    // (on the stream of the patch kernels: a fill on the null stream is not ordered against the non-blocking side
    // stream of a fused stress launch and could wipe rows its kernels have already written)
    HIP_TRY(hipMemsetAsync(h->bt.slots, 0, bytes, st));
    h->slots_first_bin = eqlb::MAX_BINS;
  }
  // The reduction adds ALL slot rows of a cell.  A run over a part of the patches rewrites only their rows: rows
  // of the others left by an earlier run over more of them (option "scatter" / "solver" changed on this handle)
  // would be added again on top of what the tiled launch wrote
  if (h->slots_first_bin < cover)
    HIP_TRY(hipMemsetAsync(h->bt.slots, 0, bytes, st));
  h->slots_first_bin = cover;
  return EQLB_OK;
}

// Patch kernels of a range on stream st: rows into the slot buffer (scatter = SLOTS) or added to flux_hdiv by fp64
// atomics (ATOMIC).  All bins in one launch where that kernel exists (timing slot of bin 0), else one launch per bin.
int launch_patches(const Sweep& s, const PatchRange& pr, int scatter, hipStream_t st, const eqlb::DevEvent* evs)
{
  const eqlb_se* h = s.h;
  const bool to_slots = scatter == EQLB_SCATTER_SLOTS;
  eqlb::SeArgs as = s.a;
  if ((h->mode == 1 && h->k <= 3) || (h->fused && h->solver == EQLB_SOLVER_SHUFFLE && h->k <= 3))
  {
    eqlb::FusedBins fb{};
    int64_t nb = 0;
    for (int b = 0; b < eqlb::MAX_BINS; ++b)
    {
      fb.block_start[b] = nb;
      fb.npatch[b] = pr.npatch[b];
      fb.slot_offset[b] = pr.slot_offset[b];
      fb.patch_offset[b] = pr.patch_offset[b];
      nb += (pr.npatch[b] * h->bt.bins[b].P + 255) / 256;
    }
    fb.block_start[eqlb::MAX_BINS] = nb;
    for (int r = 0; r < h->nrhs; ++r)
    {
      select_rhs(s, as, r, to_slots);
      if (r == 0)
        EQLB_TRY(mark_begin(evs, eqlb_se::EV_BIN0, st));
      const int st_ = (h->mode == 1) ? eqlb::launch_ev_patch_fused(h->k, h->deg, as, fb, st)
                                     : eqlb::launch_se_patch_fused(h->k, h->deg, scatter, as, fb, st);
      if (st_)
        return fail(st_, "fused patch kernel launch failed (k=%d)", h->k);
    }
    return mark_end(evs, eqlb_se::EV_BIN0, st);
  }
  // (EV is refused with the atomic scatter: those launches carry no mode)
  const int mode = to_slots ? h->mode : 0;
  for (int b = 0; b < eqlb::MAX_BINS; ++b)
  {
    if (pr.npatch[b] == 0)
      continue;
    as.npatch = pr.npatch[b];
    as.slot_offset = pr.slot_offset[b];
    as.patch_offset = pr.patch_offset[b];
    EQLB_TRY(mark_begin(evs, eqlb_se::EV_BIN0 + b, st));
    for (int r = 0; r < h->nrhs; ++r)
    {
      select_rhs(s, as, r, to_slots);
      const int st_ = eqlb::launch_se_patch(h->k, h->deg, h->bt.bins[b].P, h->solver, scatter, as, st, mode);
      if (st_)
        return fail(st_, "patch kernel launch failed (k=%d, P=%d)", h->k, h->bt.bins[b].P);
    }
    EQLB_TRY(mark_end(evs, eqlb_se::EV_BIN0 + b, st));
  }
  return EQLB_OK;
}

// Patches of more than 63 cells: one workgroup each, rows into the slot buffer (rewritten by every call)
int launch_large(const Sweep& s, hipStream_t st, const eqlb::DevEvent* evs)
{
  const eqlb_se* h = s.h;
  eqlb::SeArgs al = s.a;
  al.slot_cell = h->bt.l_slot_cell;
  al.slot_info = h->bt.l_slot_info;
  al.pn = nullptr;
  al.pflag = h->bt.l_pflag;
  al.npatch_total = h->bt.l_npatch;
  EQLB_TRY(mark_begin(evs, eqlb_se::EV_LARGE, st));
  for (int r = 0; r < h->nrhs; ++r)
  {
    select_rhs(s, al, r, true);
    const int st_ = eqlb::launch_se_patch_large(h->k, h->deg, h->mode, al, h->bt.l_off, h->bt.l_ws, st);
    if (st_)
      return fail(st_, "large-patch kernel launch failed (k=%d)", h->k);
  }
  return mark_end(evs, eqlb_se::EV_LARGE, st);
}

// Weak symmetry of rows 0, 1 on the large patches: one launch for all of them, behind launch_large (it corrects the slot
// rows that kernel wrote) and before the reduction that consumes them.  Timing slot of the weak-symmetry kernels:
// `begin` opens it, else the launch extends the slot that launch_weaksym has opened on this stream
int launch_weaksym_large(const Sweep& s, hipStream_t st, const eqlb::DevEvent* evs, bool begin)
{
  const eqlb_se* h = s.h;
  eqlb::SeArgs al = s.a;
  al.slot_cell = h->bt.l_slot_cell;
  al.slot_info = h->bt.l_slot_info;
  al.pn = nullptr;
  al.pflag = h->bt.l_pflag;
  al.npatch_total = h->bt.l_npatch;
  select_rhs(s, al, 0, true);
  al.tables = h->tables + eqlb::table_offset_te(h->k, h->deg) - eqlb::table_offset_te(h->k, h->k - 1); // as launch_weaksym
  if (begin)
    EQLB_TRY(mark_begin(evs, eqlb_se::EV_WEAKSYM, st));
  const int st_ = eqlb::launch_se_weaksym_large(h->k, al, h->bt.l_off, h->bt.l_wsym_off, h->bt.l_wsym_ws, st);
  if (st_)
    return fail(st_, "weak-symmetry kernel launch of the large patches failed (k=%d)", h->k);
  return mark_end(evs, eqlb_se::EV_WEAKSYM, st);
}

// Weak symmetry of rows 0, 1 on the patch-local stresses held in the slots
// (se/reconstruction.hpp:237-270; the grouped boundary patches of :170-234 are flagged by the
// patch builder: PFLAG_WS_SKIP / PFLAG_WS_GROUP)
int launch_weaksym(const Sweep& s, const PatchRange& pr, hipStream_t st, const eqlb::DevEvent* evs)
{
  const eqlb_se* h = s.h;
  EQLB_TRY(mark_begin(evs, eqlb_se::EV_WEAKSYM, st));
  eqlb::SeArgs as = s.a;
  select_rhs(s, as, 0, true); // the kernel works on the slot rows of RHS 0 and 1
  // the weak-symmetry kernels address the tensors TE ... VQ of the table buffer by the offsets of DG_{k-1}: with
  // data of a lower degree the segments in front of them (F, H, D) are shorter, the base pointer moves by the
  // difference (every read stays inside the buffer; TE ... VQ do not depend on the degree)
  as.tables = h->tables + eqlb::table_offset_te(h->k, h->deg) - eqlb::table_offset_te(h->k, h->k - 1);
  // (overlapping groups of boundary patches: one pass per level, a pass skips the patches of other levels)
  for (int lv = 0; lv < h->bt.ws_levels; ++lv)
    for (int b = 0; b < eqlb::MAX_BINS; ++b)
    {
      if (pr.npatch[b] == 0)
        continue;
      as.npatch = pr.npatch[b];
      as.slot_offset = pr.slot_offset[b];
      as.patch_offset = pr.patch_offset[b];
      as.ws_level = lv;
      const int st_ = eqlb::launch_se_weaksym(h->k, h->bt.bins[b].P, !h->bt.stress_flux_bcs && h->deg == h->k - 1, as, st);
      if (st_)
        return fail(st_, "weak-symmetry kernel launch failed (k=%d, P=%d)", h->k, h->bt.bins[b].P);
    }
  return mark_end(evs, eqlb_se::EV_WEAKSYM, st);
}

// Reduction of all slot rows of every cell into the output (EV: to the conforming DOFs)
int reduce_all(const Sweep& s, hipStream_t st)
{
  const eqlb_se* h = s.h;
  // blocks that lie behind one another (one array, the usual case) are reduced by one launch
  bool contiguous = true;
  for (int r = 1; r < h->nrhs; ++r)
    contiguous = contiguous && s.d_x[r] == s.d_x[0] + r * s.s_x;
  const int nlaunch = contiguous ? 1 : h->nrhs, per = contiguous ? h->nrhs : 1;
  for (int l = 0; l < nlaunch; ++l)
  {
    const double* sl = h->bt.slots + (size_t)l * s.s_slot * 3;
    if (s.ev_conf)
      eqlb::launch_ev_reduce(s.m, h->k, per, h->ev_cell_dofs, h->ev_ndofs, sl, s.d_x[l], h->accumulate, h->ev_basis,
                             basis_R(h), st);
    else if (eqlb::launch_reduce_slots(h->nrt, s.m.ncells, per, sl, s.d_x[l], h->accumulate, st))
      return fail(EQLB_ERR_UNSUPPORTED, "slot reduction for %d DOFs per cell is not in this build", h->nrt);
  }
  return EQLB_OK;
}

// Compact reduction: the slot rows of the listed cells are ADDED to the output (the rows of their other vertices are
// zero).  (EV, conforming output: k_ev_reduce runs over the whole mesh - 3 nrt doubles per cell and right-hand side,
// zeros but for the listed cells, correct and in fixed order; a conforming reduction over a cell list and its facets
// is the follow-up)
int reduce_cells(const Sweep& s, int64_t nlist, const int32_t* cells, hipStream_t st)
{
  const eqlb_se* h = s.h;
  for (int r = 0; r < h->nrhs; ++r)
  {
    const double* sl = h->bt.slots + (size_t)r * s.s_slot * 3;
    if (s.ev_conf)
      eqlb::launch_ev_reduce(s.m, h->k, 1, h->ev_cell_dofs, h->ev_ndofs, sl, s.d_x[r], 1, h->ev_basis, basis_R(h), st);
    else if (eqlb::launch_reduce_slots_cells(h->nrt, s.m.ncells, nlist, cells, sl, s.d_x[r], st))
      return fail(EQLB_ERR_UNSUPPORTED, "compact slot reduction for %d DOFs per cell is not in this build", h->nrt);
  }
  return EQLB_OK;
}

// ---- slot route: (cell, vertex) rows into the slot buffer, weak symmetry on the slot rows, reduction ----
int sweep_slots(const Sweep& s)
{
  const eqlb_se* h = s.h;
  const PatchRange pr = all_patches(h);
  EQLB_TRY(ensure_slots(s, COVER_ALL, s.stream));
  EQLB_TRY(launch_patches(s, pr, EQLB_SCATTER_SLOTS, s.stream, s.evs));
  if (h->bt.l_npatch > 0)
    EQLB_TRY(launch_large(s, s.stream, s.evs));
  if (h->stress)
    EQLB_TRY(launch_weaksym(s, pr, s.stream, s.evs));
  if (h->stress && h->bt.l_npatch > 0)
    EQLB_TRY(launch_weaksym_large(s, s.stream, s.evs, false));
  EQLB_TRY(mark_begin(s.evs, eqlb_se::EV_REDUCE, s.stream));
  EQLB_TRY(reduce_all(s, s.stream));
  return mark_end(s.evs, eqlb_se::EV_REDUCE, s.stream);
}

// ---- atomic route: fp64 global atomics straight into flux_hdiv ----
int sweep_atomic(const Sweep& s)
{
  return launch_patches(s, all_patches(s.h), EQLB_SCATTER_ATOMIC, s.stream, s.evs);
}

// The right-hand sides r0 ... nrhs - 1 on the tiles: one launch per chunk of MULTI_RHS_MAX (option "multi_rhs") or
// one per right-hand side
int launch_tiled_rhs(const Sweep& s, eqlb::SeArgs& at, const eqlb::TileArgs& ta, int r0)
{
  const eqlb_se* h = s.h;
  if (h->multi_rhs && h->nrhs - r0 > 1)
  {
    for (int rb = r0; rb < h->nrhs; rb += eqlb::MULTI_RHS_MAX)
    {
      eqlb::MultiRhs mr{};
      mr.n = std::min(eqlb::MULTI_RHS_MAX, h->nrhs - rb);
      mr.rhs0 = rb;
      for (int i = 0; i < mr.n; ++i)
      {
        mr.g[i] = s.d_g[rb + i];
        mr.f[i] = s.d_f[rb + i];
        mr.x[i] = s.d_x[rb + i];
      }
      select_rhs(s, at, rb, false);
      const int st = eqlb::launch_se_patch_tiled_multi(h->k, h->deg, h->mode, at, ta, mr, s.stream);
      if (st)
        return fail(st, "tiled multi-RHS patch kernel launch failed (k=%d)", h->k);
    }
    return EQLB_OK;
  }
  for (int r = r0; r < h->nrhs; ++r)
  {
    select_rhs(s, at, r, false);
    const int st = eqlb::launch_se_patch_tiled(h->k, h->deg, h->mode, at, ta, s.stream);
    if (st)
      return fail(st, "tiled patch kernel launch failed (k=%d)", h->k);
  }
  return EQLB_OK;
}

// ---- tiled route: one workgroup per tile of cells, no slot buffer.  Timing slot of bin 0: all tiled launches ----
int sweep_tiled(const Sweep& s)
{
  eqlb_se* h = s.h;
  const int32_t tcount = (h->tile_count < 0) ? h->bt.ntiles - h->tile_first
                                             : std::min(h->tile_count, h->bt.ntiles - h->tile_first);
  const eqlb::TileArgs ta{h->bt.t_tiles, h->bt.t_tile_cells, tcount, h->bt.tile_tc,
                          s.ev_conf ? h->bt.t_facet_owner : nullptr, h->ev_cell_dofs, h->ev_ndofs, s.m.nfacets,
                          h->tile_first, h->accumulate, s.ev_conf ? h->ev_basis : nullptr,
                          s.ev_conf ? basis_R(h) : nullptr};
  eqlb::SeArgs at = s.a;
  at.slot_cell = h->bt.t_slot_cell;
  at.slot_info = h->bt.t_slot_info;
  at.pn = h->bt.t_pn;
  at.pflag = h->bt.t_pflag;
  at.npatch_total = h->bt.t_npatch;
  EQLB_TRY(mark_begin(s.evs, eqlb_se::EV_BIN0, s.stream));
  // What the tiles leave out - the rest of a fused stress launch, the large patches - goes along with the FIRST range
  // of tiles of a two-phase sweep: its patches touch ghost cells like any other, and the caller packs the ghost rows
  // behind that range (option accumulate = 0: the tiled launches STORE, the sums can only be added behind the last of
  // them; an empty range - a rank without priority tiles, or with priority tiles only - takes nothing along)
  const bool with_first_range = tcount > 0 && (h->accumulate ? h->tile_first == 0 : h->tile_first + tcount == h->bt.ntiles);
  // The rest of a fused stress launch (boundary patches, interior patches that are not full, bins of more than 8
  // lanes): its patch kernels - a handful of small launches, 50 us back to back at 1M triangles - run on a side
  // stream NEXT TO the fused kernel, untimed; their sums are added behind it
  // The large patches of a stress handle go the same way, behind the rest: flux rows, then their weak symmetry (both
  // timed: the slots of the large-patch kernel and of the weak-symmetry kernels)
  const bool large_now = h->bt.l_npatch > 0 && with_first_range;
  const bool rest_now = s.stress_fused && with_first_range && (h->bt.t_rest > 0 || large_now);
  if (rest_now)
  {
    if (!h->side.stream)
    {
      eqlb_se::SideLane lane;
      HIP_TRY(lane.stream.create(hipStreamNonBlocking));
      HIP_TRY(lane.fork.create(hipEventDisableTiming));
      HIP_TRY(lane.join.create(hipEventDisableTiming));
      h->side = std::move(lane);
    }
    const PatchRange rest = rest_of_fused_stress(h);
    HIP_TRY(hipEventRecord(h->side.fork, s.stream));
    HIP_TRY(hipStreamWaitEvent(h->side.stream, h->side.fork, 0));
    EQLB_TRY(ensure_slots(s, COVER_REST, h->side.stream));
    if (h->bt.t_rest > 0)
    {
      EQLB_TRY(launch_patches(s, rest, EQLB_SCATTER_SLOTS, h->side.stream, nullptr));
      EQLB_TRY(launch_weaksym(s, rest, h->side.stream, nullptr));
    }
    if (large_now)
    {
      EQLB_TRY(launch_large(s, h->side.stream, s.evs));
      EQLB_TRY(launch_weaksym_large(s, h->side.stream, s.evs, true));
    }
    HIP_TRY(hipEventRecord(h->side.join, h->side.stream));
  }
  int r0 = 0;
  if (s.stress_fused)
  {
    // rows 0, 1 of the stress and their weak symmetry in one launch
    select_rhs(s, at, 0, false);
    const int st = eqlb::launch_se_stress_tiled(at, ta, s.d_g, s.d_f, s.d_x, s.stream, h->bt.t_mixed);
    if (st)
      return fail(st, "fused stress kernel launch failed");
    r0 = 2;
  }
  EQLB_TRY(launch_tiled_rhs(s, at, ta, r0));
  EQLB_TRY(mark_end(s.evs, eqlb_se::EV_BIN0, s.stream));
  if (large_now && !s.stress_fused)
  {
    // The tiles treat the node of a large patch like a masked node (TileDesc::zero): its rows are missing from what
    // they wrote.  The large-patch kernel puts them into the slot buffer - every other row of it is zero - and a
    // compact reduction over the cells of those patches ADDS them behind the tiles
    EQLB_TRY(ensure_slots(s, COVER_LARGE, s.stream));
    EQLB_TRY(launch_large(s, s.stream, s.evs));
    EQLB_TRY(reduce_cells(s, h->bt.l_ncells, h->bt.l_cells, s.stream));
  }
  if (rest_now)
  {
    // only the cells that a patch of the generic kernels touches
    HIP_TRY(hipStreamWaitEvent(s.stream, h->side.join, 0));
    if (large_now)
      EQLB_TRY(reduce_cells(s, h->bt.l_nrest_cells, h->bt.l_rest_cells, s.stream));
    else
      EQLB_TRY(reduce_cells(s, h->bt.nrest_cells, h->bt.rest_cells, s.stream));
  }
  return EQLB_OK;
}

// The sweep on per-right-hand-side arrays: g[r], f[r], x[r] are the blocks of RHS r (host or device).
int equilibrate_lists(eqlb_se_t* h, const double* const* g_in, const double* const* f_in, double* const* x_io,
                      int32_t memspace, void* stream_)
{
  if (!h || !g_in || !f_in || !x_io)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "Equilibration: Input sizes does not match");
  for (int r = 0; r < h->nrhs; ++r)
    if (!g_in[r] || !f_in[r] || !x_io[r])
      return fail(EQLB_ERR_INVALID_ARGUMENT, "Equilibration: Input sizes does not match");
  if (!h->bt.boundary_set)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_equilibrate: boundary data not set");
  const eqlb::DeviceMesh& m = h->mesh->m;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  int scatter = 0;
  bool stress_fused = false;
  EQLB_TRY(plan_sweep(h, scatter, stress_fused));
  const bool ev_conf = h->mode == 1 && h->ev_output == 0;
  const size_t s_g = (size_t)m.ncells * h->nd * 2, s_f = (size_t)m.ncells * h->nd, s_slot = (size_t)m.ncells * h->nrt;
  const size_t s_x = ev_conf ? (size_t)h->ev_ndofs : s_slot;

  std::vector<const double*> d_g(g_in, g_in + h->nrhs), d_f(f_in, f_in + h->nrhs);
  std::vector<double*> d_x(x_io, x_io + h->nrhs);
  EQLB_TRY(eqlb::check_memspace("eqlb_se_equilibrate", memspace));
  if (memspace == EQLB_MEM_HOST)
    EQLB_TRY(stage_in(h, s_g, s_f, s_x, g_in, f_in, x_io, d_g.data(), d_f.data(), d_x.data(), stream));

  const eqlb::DevEvent* evs = nullptr;
  if (h->timing)
    EQLB_TRY(timing_events(h, evs));

  eqlb::SeArgs a{};
  a.cellJ = m.cellJ;
  a.slot_cell = h->bt.slot_cell;
  a.slot_info = h->bt.slot_info;
  a.pn = h->bt.pn;
  a.pflag = h->bt.pflag;
  a.tables = h->tables;
  a.bvals = h->bt.bvals;
  a.status = h->status;
  a.npatch_total = h->bt.npatch_total;
  a.ncells = m.ncells;
  a.nrhs = h->nrhs;
  const Sweep s{h, m, stream, scatter, stress_fused, ev_conf, s_g, s_f, s_slot, s_x, d_g.data(), d_f.data(), d_x.data(),
                a, evs};
  const int st = (scatter == EQLB_SCATTER_TILED)   ? sweep_tiled(s)
                 : (scatter == EQLB_SCATTER_SLOTS) ? sweep_slots(s)
                                                   : sweep_atomic(s);
  if (st)
    return st;
  if (evs)
    ++h->ev_calls;
  // patches of a cell of zero area were left out (eqlb_se_set_boundary): the call reports them like a patch system that
  // is not positive definite, behind its kernels on the caller's stream
  if (h->bt.flat_swept)
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(static_cast<int32_t*>(h->status)), 1, 1, stream));
  HIP_TRY(hipGetLastError());
  if (memspace == EQLB_MEM_HOST)
    return stage_out(h, s_x, x_io, d_x.data(), stream);
  return EQLB_OK;
}
} // namespace

extern "C" {

int eqlb_se_equilibrate_lists(eqlb_se_t* h, const double* const* flux_dg, const double* const* rhs_dg,
                              double* const* flux_hdiv, int32_t memspace, void* stream)
try
{
  return equilibrate_lists(h, flux_dg, rhs_dg, flux_hdiv, memspace, stream);
}
EQLB_CATCH_ALL

int eqlb_se_equilibrate(eqlb_se_t* h, const double* flux_dg, const double* rhs_dg,
                        double* flux_hdiv, int32_t memspace, void* stream_)
try
{
  if (!h || !flux_dg || !rhs_dg || !flux_hdiv)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "Equilibration: Input sizes does not match");
  const eqlb::DeviceMesh& m = h->mesh->m;
  const size_t s_g = (size_t)m.ncells * h->nd * 2, s_f = (size_t)m.ncells * h->nd;
  const size_t s_x = (h->mode == 1 && h->ev_output == 0) ? (size_t)h->ev_ndofs : (size_t)m.ncells * h->nrt;
  std::vector<const double*> g(h->nrhs), f(h->nrhs);
  std::vector<double*> x(h->nrhs);
  for (int r = 0; r < h->nrhs; ++r)
  {
    g[r] = flux_dg + r * s_g;
    f[r] = rhs_dg + r * s_f;
    x[r] = flux_hdiv + r * s_x;
  }
  return equilibrate_lists(h, g.data(), f.data(), x.data(), memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_se_equilibrate_with_kornconst(eqlb_se_t* h, const double* flux_dg, const double* rhs_dg,
                                       double* flux_hdiv, double* cells_kornconst,
                                       int32_t memspace, void* stream_)
try
{
  if (!cells_kornconst)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "Equilibration: Input sizes does not match");
  const int st = eqlb_se_equilibrate(h, flux_dg, rhs_dg, flux_hdiv, memspace, stream_);
  if (st)
    return st;
  return eqlb_se_kornconst(h, cells_kornconst, memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_se_equilibrate_tiles(eqlb_se_t* h, const double* flux_dg, const double* rhs_dg, double* flux_hdiv,
                              int32_t tile_first, int32_t tile_count, void* stream)
try
{
  if (!h || tile_first < 0)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_equilibrate_tiles: invalid argument");
  const int32_t f0 = h->tile_first, c0 = h->tile_count;
  h->tile_first = tile_first;
  h->tile_count = tile_count;
  const int st = eqlb_se_equilibrate(h, flux_dg, rhs_dg, flux_hdiv, EQLB_MEM_DEVICE, stream);
  h->tile_first = f0;
  h->tile_count = c0;
  return st;
}
EQLB_CATCH_ALL

int eqlb_se_check_status(eqlb_se_t* h, void* stream_)
{
  if (!h)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_se_check_status: null handle");
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  int32_t status = 0;
  HIP_TRY(hipMemcpyAsync(&status, h->status, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  if (status)
  {
    HIP_TRY(hipMemsetAsync(h->status, 0, sizeof(int32_t), stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return fail(EQLB_ERR_SINGULAR, "patch system not positive definite");
  }
  return EQLB_OK;
}

double eqlb_se_last_kernel_ms(const eqlb_se_t* h, int32_t which)
{
  // which: a timing slot (eqlb_se::EvSlot) - b (0..4): patch kernel of bin b (P = 4 << b); 5: slot reduction;
  // 6: weak-symmetry kernels; 7: large-patch kernel.
  // Average device time per launch over the calls recorded since timing was enabled
  // (at most the last EV_RING calls).  Synchronises with the recorded events.
  if (!h || h->ev.empty() || h->ev_calls == 0 || which < 0 || which >= eqlb_se::EV_NSLOTS)
    return 0.0;
  if (which == eqlb_se::EV_WEAKSYM && !h->stress)
    return 0.0;
  if (which == eqlb_se::EV_LARGE && (h->bt.l_npatch == 0 || h->scatter_last == EQLB_SCATTER_ATOMIC))
    return 0.0; // the large-patch kernel (all right-hand sides of a call)
  const bool fused_run = (h->mode == 1 && h->k <= 3) || h->scatter_last == EQLB_SCATTER_TILED
                         || (h->fused && h->solver == EQLB_SOLVER_SHUFFLE && h->k <= 3);
  if (which < eqlb::MAX_BINS && ((fused_run && which != 0) || (!fused_run && h->bt.bins[which].npatch == 0)))
    return 0.0;
  if (which == eqlb_se::EV_REDUCE && h->scatter_last != EQLB_SCATTER_SLOTS)
    return 0.0;
  const int64_t nset = std::min<int64_t>(h->ev_calls, eqlb_se::EV_RING);
  double sum = 0.0;
  for (int64_t s = 0; s < nset; ++s)
  {
    const eqlb::DevEvent* evs = h->ev.data() + s * eqlb_se::EV_PER_SET;
    float ms = 0.f;
    if (hipEventSynchronize(evs[eqlb_se::ev_end(which)]) != hipSuccess
        || hipEventElapsedTime(&ms, evs[eqlb_se::ev_begin(which)], evs[eqlb_se::ev_end(which)]) != hipSuccess)
      return 0.0;
    sum += ms;
  }
  return sum / (double)nset;
}

// the same entries of an EV handle
int eqlb_ev_equilibrate(eqlb_ev_t* h, const double* flux_dg, const double* rhs_dg,
                        double* flux_hdiv, int32_t memspace, void* stream)
try
{
  if (!h)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "Equilibration: Input sizes does not match");
  return eqlb_se_equilibrate(h->se.get(), flux_dg, rhs_dg, flux_hdiv, memspace, stream);
}
EQLB_CATCH_ALL

int eqlb_ev_equilibrate_lists(eqlb_ev_t* h, const double* const* flux_dg, const double* const* rhs_dg,
                              double* const* flux_hdiv, int32_t memspace, void* stream)
try
{
  if (!h)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "Equilibration: Input sizes does not match");
  return eqlb_se_equilibrate_lists(h->se.get(), flux_dg, rhs_dg, flux_hdiv, memspace, stream);
}
EQLB_CATCH_ALL

int eqlb_ev_check_status(eqlb_ev_t* h, void* stream)
{
  if (!h)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_ev_check_status: null handle");
  return eqlb_se_check_status(h->se.get(), stream);
}

double eqlb_ev_last_kernel_ms(const eqlb_ev_t* h, int32_t which)
{
  return h ? eqlb_se_last_kernel_ms(h->se.get(), which) : 0.0;
}

} // extern "C"
