// The tiled launch of se_patch_body (eqlb_se_body.h): staging of a tile, the sweep over its patches, the flush of
// its rows, the two kernels and their launchers by template arguments.  Instantiated by eqlb_se_kernels.hip
// (DEG = k - 1), eqlb_se_kernels_lowdeg.hip and eqlb_se_kernels_pair.hip.
#pragma once

#include "eqlb_se_body.h"

namespace eqlb
{

// ---- tiled launch: no slot buffer, no reduction pass ----------------------------------------------
// One workgroup (8 waves) per tile of TC owned cells.  It solves every patch that touches an owned
// cell (patches on the tile rim are solved by each tile they touch), writes the (cell, vertex) rows
// of its OWN cells into LDS - every row exactly once, no atomics - and finally adds
// row(v0) + row(v1) + row(v2) in fixed order to flux_hdiv: bitwise reproducible from run to run.
// k <= 2: 8 waves own EQLB_TILE_CELLS cells (two workgroups per CU); k = 3: 8 waves, EQLB_TILE_CELLS_K3 cells (one per CU)
constexpr int tile_threads_c(int k) { return (k >= 3) ? EQLB_TILE_THREADS_K3 : EQLB_TILE_THREADS; }
// (k = 3, measured at 1M triangles: 256 threads / 160 cells 0.384 ms, 512 / 320 0.366, 512 / 440 0.339; the tile builder
// picks the size that fills whole rounds of the 256 slots)
constexpr int tile_cells_c(int k) { return (k >= 3) ? EQLB_TILE_CELLS_K3 : EQLB_TILE_CELLS; }
// largest tile the LDS budget of two workgroups per CU allows (k <= 2: 490 x 144 B + tensors <= 80 KB)
constexpr int tile_cells_max_c(int k) { return (k >= 3) ? EQLB_TILE_CELLS_K3 : (EQLB_TILE_CELLS > 490 ? EQLB_TILE_CELLS : 490); }

// MODE 0: semi-explicit flux, flux_hdiv in the broken layout.  MODE 1: EV patch problems; flush to
// the conforming DOFs (ta.facet_owner != nullptr) or to the broken layout ("output" = 1).
// bijective XCD swizzle: block b of n -> position of b in the order
// "all blocks of XCD label 0, then of label 1, ..."
__device__ __forceinline__ int xcd_remap(int b, int n)
{
  const int q = n / 8, r = n % 8, x = b % 8;
  return ((x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q) + b / 8;
}

// DOF i of a cell from its three packed (cell, vertex) rows in LDS: row(v0) + row(v1) + row(v2) in this
// order (the order of the slot path); a facet DOF gets nothing from the vertex opposite to its facet
template <int K, int NPK>
__device__ __forceinline__ double packed_sum(const double* rows, int i)
{
  if (i >= 3 * K) // interior DOFs: all three rows
  {
    const int q = i - K;
    return (rows[q] + rows[NPK + q]) + rows[2 * NPK + q];
  }
  const int f = i / K, j = i - f * K;
  // rows ln != f, ascending; position of facet f in row ln: f - (f > ln)
  const int la = (f == 0) ? 1 : 0, lb = (f == 2) ? 1 : 2;
  return rows[la * NPK + (f - ((f > la) ? 1 : 0)) * K + j] + rows[lb * NPK + (f - ((f > lb) ? 1 : 0)) * K + j];
}

// first half of a tile: the reference tensors into LDS (and the zeroing of the slots where a node mask leaves
// rows unwritten), ends with the workgroup barrier
template <int K, int DEG, int MODE>
__device__ __forceinline__ void tile_stage(const SeArgs& a0, const TileArgs& ta, const int tile, double* lds)
{
  constexpr int TILE_THREADS = tile_threads_c(K);
  using Z = Sizes<K, DEG, 8>;
  constexpr int NRT = Z::NRT;
  const int TC = ta.tc;
  constexpr int NPK = NRT - K; // packed (cell, vertex) row: without the facet opposite to the vertex
  constexpr bool HALFWQ = K == 3; // as in se_patch_body
  constexpr int NTABL = HALFWQ ? Z::NTAB_HALF : Z::NTAB;
  constexpr int NTABM = NTABL + (MODE ? Z::NEV : 0);
  double* sSlots = lds + NTABM;
  if constexpr (HALFWQ)
  {
    constexpr int NHEAD = Z::NF + Z::NHT + Z::NDT + Z::NTET; // F | H | D | TE
    constexpr int NCMB = Z::NCMB;                            // one combination of WQ (NCMBH: its padded stride in LDS)
    for (int i = threadIdx.x; i < NHEAD; i += TILE_THREADS)
      lds[i] = a0.tables[Z::NS + i];
    for (int i = threadIdx.x; i < (NCOMBO / 2) * NCMB; i += TILE_THREADS) // combinations 0, 2, 4, ...: no reversal
      lds[NHEAD + (i / NCMB) * Z::NCMBH + (i % NCMB)] = a0.tables[Z::NS + NHEAD + (i / NCMB) * 2 * NCMB + (i % NCMB)];
    for (int i = threadIdx.x; i < Z::NHB; i += TILE_THREADS)
      lds[NHEAD + Z::NWQH + i] = a0.tables[Z::NS + NHEAD + Z::NWQT + i];
  }
  else
    for (int i = threadIdx.x; i < Z::NTAB; i += TILE_THREADS)
      lds[i] = a0.tables[Z::NS + i];
  if constexpr (MODE == 1)
    for (int i = threadIdx.x; i < Z::NEV; i += TILE_THREADS)
      lds[NTABL + i] = a0.tables[Z::OFF_HG + i];
  // every packed row of an owned cell is written completely by the patch of its vertex; rows of
  // vertices that this rank does not equilibrate (node mask; flagged per tile) must read as zero in
  // the flush
  if (ta.tiles[tile].zero)
    for (int i = threadIdx.x; i < TC * 3 * NPK; i += TILE_THREADS)
      sSlots[i] = 0.0;
  __syncthreads();
}

// one wave-block of 16 full 8-cell patches on four lanes per patch, two ring cells per lane (eqlb_se_kernels_pair.hip);
// slot_base: the first slot of the wave-block in the lane space of the bin (wave-uniform), lane: the lane of the wave
template <int K, int DEG>
__device__ void se_pair_body(const SeArgs& a, int64_t slot_base, int lane, double* lds, double* tile_slots);

// second half: every patch of the tile for ONE right-hand side (a0.rhs, a0.flux_dg, a0.rhs_dg, a0.out), then the
// flush of the tile's rows.  PAIR: the leading full patches of the bin P = 8 run in wave-blocks of 16 on se_pair_body,
// the remainder of fewer than 16 on the full-patch instance below, 8 per wave-block
template <int K, int DEG, int MODE, bool PAIR = false>
__device__ __forceinline__ void tile_sweep_flush(const SeArgs& a0, const TileArgs& ta, const int tile, double* lds)
{
  constexpr int TILE_THREADS = tile_threads_c(K);
  using Z = Sizes<K, DEG, 8>;
  constexpr int NRT = Z::NRT;
  constexpr int TCMAX = tile_cells_max_c(K); // sizes the register arrays of the flush
  const int TC = ta.tc;                      // cells per tile of this SoA (<= TCMAX)
  constexpr int NPK = NRT - K;
  constexpr bool HALFWQ = K == 3;
  constexpr int NTABL = HALFWQ ? Z::NTAB_HALF : Z::NTAB;
  constexpr int NTABM = NTABL + (MODE ? Z::NEV : 0);
  double* sSlots = lds + NTABM;
  const TileDesc& td = ta.tiles[tile];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  constexpr int NW = TILE_THREADS / 64;
  int u = wave;
  if constexpr (PAIR) // (the wave-block counter as well)
    u = __builtin_amdgcn_readfirstlane(u);
  SeArgs a = a0;
  // (PAIR: the counts of the tile as wave-uniform values in scalar registers - that kernel has no vector register to spare)
#define EQLB_TILE_UNI(x) (PAIR ? __builtin_amdgcn_readfirstlane(x) : (x))
#define EQLB_TILE_BIN(B, PP)                                                                        \
  {                                                                                                 \
    const int np = EQLB_TILE_UNI(td.npatch[B]);                                                     \
    const int nwb = tile_wb_all(np, PP);                                                            \
    a.npatch = np;                                                                                  \
    a.slot_offset = EQLB_TILE_UNI(td.slot_start[B]);                                                \
    a.patch_offset = EQLB_TILE_UNI(td.patch_start[B]);                                              \
    /* (every instance on the register solver, SOLVER 1) */                                         \
    /* complete wave-blocks of full patches (RT_1: the body is too small for the second instance to pay) */ \
    constexpr bool SPEC = tile_spec_full(K, PP);                                                    \
    const int nfull_b = EQLB_TILE_UNI(td.nfull[B]);                                                 \
    const int nwb_full = SPEC ? tile_wb_whole(nfull_b, PP) : 0;                                     \
    /* wave-blocks of interior patches of any size (the patches behind the full ones; K = 2, P = 8, 16) */ \
    constexpr bool SPECI = tile_spec_interior(K, PP);                                               \
    const int nwb_int = SPECI ? tile_wb_whole(EQLB_TILE_UNI(td.nint[B]), PP) : 0;                   \
    /* PAIR: units [0, npair) are wave-blocks of 16 full patches (the 64-lane blocks 2 u, 2 u + 1 of the list), */ \
    /* unit u >= npair is the 64-lane block u + npair */                                            \
    constexpr bool PAIRB = PAIR && PP == 8 && K == 2 && MODE == 0;                                  \
    const int npair = PAIRB ? (nfull_b >> 4) : 0;                                                   \
    const int nun = nwb - npair;                                                                    \
    for (; u < nun; u += NW)                                                                        \
    {                                                                                               \
      if constexpr (PAIRB)                                                                          \
        if (u < npair)                                                                              \
        {                                                                                           \
          se_pair_body<K, DEG>(a, (int64_t)u * 128, lane, lds, sSlots);                             \
          continue;                                                                                 \
        }                                                                                           \
      const int v = u + npair;                                                                      \
      if (v < nwb_full)                                                                             \
        se_patch_body<K, DEG, PP, 1, 2, 64, MODE, SPEC>(a, 0, lds, true, (int64_t)v * 64 + lane, sSlots); \
      else if (SPECI && v < nwb_int)                                                                \
        se_patch_body<K, DEG, PP, 1, 2, 64, MODE, false, SPECI>(a, 0, lds, true, (int64_t)v * 64 + lane, sSlots); \
      else                                                                                          \
        se_patch_body<K, DEG, PP, 1, 2, 64, MODE>(a, 0, lds, true, (int64_t)v * 64 + lane, sSlots); \
    }                                                                                               \
    u -= nun;                                                                                       \
  }
  EQLB_TILE_BIN(0, 4)
  EQLB_TILE_BIN(1, 8)
  EQLB_TILE_BIN(2, 16)
  EQLB_TILE_BIN(3, 32)
  EQLB_TILE_BIN(4, 64)
#undef EQLB_TILE_BIN
#undef EQLB_TILE_UNI
  const int32_t* cells = ta.tile_cells + (int64_t)tile * TC;
  const bool conforming = MODE == 1 && ta.facet_owner != nullptr;
  // flush operands of the broken layout: the old values of flux_hdiv are fetched BEFORE the barrier
  // (only this tile writes them), so that the two dependent loads hide behind the waves still solving
  double* x = a0.out + (int64_t)a0.rhs_out * a0.ncells * NRT;
  // (two consecutive DOFs per thread where the row length is even: 16-byte loads and stores)
  constexpr int VW = (NRT % 2 == 0) ? 2 : 1;
  constexpr int NIT = (TCMAX * NRT / VW + TILE_THREADS - 1) / TILE_THREADS;
  double xv[NIT][VW];
  int64_t xi[NIT];
  if (!conforming)
  {
#pragma unroll
    for (int it = 0; it < NIT; ++it)
    {
      const int e = (it * TILE_THREADS + threadIdx.x) * VW;
      const int cl = e / NRT, i = e - cl * NRT;
      const int32_t cell = (e < TC * NRT) ? cells[cl] : -1;
      xi[it] = (cell >= 0) ? (int64_t)cell * NRT + i : -1;
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it)
    {
      if (!ta.accumulate) // store instead of add: the old values are not read (wave-uniform)
      {
        xv[it][0] = xv[it][VW - 1] = 0.0;
        continue;
      }
      if constexpr (VW == 2)
      {
        const double2 t = (xi[it] >= 0) ? *reinterpret_cast<const double2*>(x + xi[it]) : make_double2(0.0, 0.0);
        xv[it][0] = t.x;
        xv[it][1] = t.y;
      }
      else
        xv[it][0] = (xi[it] >= 0) ? x[xi[it]] : 0.0;
    }
  }
  // conforming layout (hierarchic basis): the owner codes, the DOF numbers and the old values of this thread's
  // facet / interior entries are fetched BEFORE the barrier as well (three dependent loads otherwise sit
  // between the barrier and the stores of every tile)
  constexpr int NIC = K * K - K;
  constexpr int NFE = (TCMAX * 3 + TILE_THREADS - 1) / TILE_THREADS;
  constexpr int NIE = (NIC > 0) ? (TCMAX * NIC + TILE_THREADS - 1) / TILE_THREADS : 1;
  int32_t fcode[NFE];
  int64_t fdof[NFE];
  double fold[NFE][K];
  int64_t idof[NIE];
  double iold[NIE];
  const bool conf_plain = conforming && ta.basis_C == nullptr;
  if (conf_plain)
  {
    const double* xc0 = a0.out + (int64_t)a0.rhs_out * ta.ndofs;
    const int32_t* own0 = ta.facet_owner + (int64_t)tile * TC * 3;
#pragma unroll
    for (int it = 0; it < NFE; ++it)
    {
      const int e = it * TILE_THREADS + threadIdx.x;
      fcode[it] = (e < TC * 3) ? own0[e] : -1;
    }
#pragma unroll
    for (int it = 0; it < NFE; ++it)
    {
      const int e = it * TILE_THREADS + threadIdx.x;
      const int cl = e / 3, lf = e - 3 * cl;
      fdof[it] = -1;
      if (fcode[it] >= 0) // facet DOFs are numbered consecutively along j (default map) or looked up per j below
        fdof[it] = ta.cell_dofs ? (int64_t)cells[cl] * NRT + lf * K : (int64_t)(fcode[it] >> 1) * K;
#pragma unroll
      for (int j = 0; j < K; ++j)
      {
        fold[it][j] = 0.0;
        if (fcode[it] >= 0 && ta.accumulate)
          fold[it][j] = ta.cell_dofs ? xc0[ta.cell_dofs[fdof[it] + j]] : xc0[fdof[it] + j];
      }
    }
    if constexpr (NIC > 0)
    {
#pragma unroll
      for (int it = 0; it < NIE; ++it)
      {
        const int e = it * TILE_THREADS + threadIdx.x;
        const int cl = e / NIC, i = e - cl * NIC;
        const int32_t cell = (e < TC * NIC) ? cells[cl] : -1;
        idof[it] = -1;
        iold[it] = 0.0;
        if (cell >= 0)
        {
          idof[it] = ta.cell_dofs ? (int64_t)ta.cell_dofs[(int64_t)cell * NRT + 3 * K + i]
                                  : (int64_t)ta.nfacets * K + (int64_t)cell * NIC + i;
          if (ta.accumulate)
            iold[it] = xc0[idof[it]];
        }
      }
    }
  }
  __syncthreads();

  if (conforming && ta.basis_C != nullptr)
  {
    // conforming DOFs of ANOTHER element basis of RT_k (the Basix space of FluxEqlbEV.py:95-100 through a
    // DOLFINx-side adapter): cell coefficients = C x broken hierarchic coefficients, facet block through R
    // where the cell sees the facet reversed; facet DOFs by the first cell of the facet
    constexpr int NI = K * K - K;
    double* xc = a0.out + (int64_t)a0.rhs_out * ta.ndofs;
    const int32_t* own = ta.facet_owner + (int64_t)tile * TC * 3;
    for (int cl = threadIdx.x; cl < TC; cl += TILE_THREADS)
    {
      const int32_t cell = cells[cl];
      if (cell < 0)
        continue;
      double c[NRT];
#pragma unroll
      for (int i = 0; i < NRT; ++i)
        c[i] = packed_sum<K, NPK>(sSlots + (int64_t)cl * 3 * NPK, i);
      // rows of C are fetched per output row inside ROLLED loops: unrolled, the compiler hoists the whole matrix
      // (k(k+2)^2 doubles) out of the cell loop and the kernel pays for the scratch it then needs on EVERY path
      auto row = [&](const int i) {
        const double* Ci = ta.basis_C + (int64_t)i * NRT;
        double s_ = 0.0;
#pragma unroll
        for (int j = 0; j < NRT; ++j)
          s_ = __builtin_fma(Ci[j], c[j], s_);
        return s_;
      };
#pragma unroll 1
      for (int lf = 0; lf < 3; ++lf)
      {
        const int32_t code = own[cl * 3 + lf];
        if (code < 0)
          continue;
        const bool rev = (code & 1) != 0 && ta.basis_R != nullptr;
        double yf[K];
#pragma unroll
        for (int j = 0; j < K; ++j)
          yf[j] = row(lf * K + j);
#pragma unroll
        for (int j = 0; j < K; ++j)
        {
          double g = yf[j];
          if (rev)
          {
            g = 0.0;
#pragma unroll
            for (int i = 0; i < K; ++i)
              g += ta.basis_R[j * K + i] * yf[i];
          }
          const int64_t dof = ta.cell_dofs ? (int64_t)ta.cell_dofs[(int64_t)cell * NRT + lf * K + j]
                                           : (int64_t)(code >> 1) * K + j;
          xc[dof] = ta.accumulate ? xc[dof] + g : g;
        }
      }
#pragma unroll 1
      for (int i = 0; i < NI; ++i)
      {
        const double yi = row(3 * K + i);
        const int64_t dof = ta.cell_dofs ? (int64_t)ta.cell_dofs[(int64_t)cell * NRT + 3 * K + i]
                                         : (int64_t)ta.nfacets * K + (int64_t)cell * NI + i;
        xc[dof] = ta.accumulate ? xc[dof] + yi : yi;
      }
    }
    return;
  }
  if (conforming)
  {
    // conforming DOFs (ev/solve_patch.hpp:223-227): facet DOFs by the first cell of the facet,
    // mapped to the global facet frame (T_f = -I / B), interior DOFs by their cell
    double* xc = a0.out + (int64_t)a0.rhs_out * ta.ndofs;
#pragma unroll
    for (int it = 0; it < NFE; ++it)
    {
      if (fcode[it] < 0)
        continue;
      const int e = it * TILE_THREADS + threadIdx.x;
      const int cl = e / 3, lf = e - 3 * cl;
      const bool rev = (fcode[it] & 1) != 0;
      double v[K];
#pragma unroll
      for (int j = 0; j < K; ++j)
        v[j] = packed_sum<K, NPK>(sSlots + (int64_t)cl * 3 * NPK, lf * K + j);
#pragma unroll
      for (int j = 0; j < K; ++j)
      {
        double g = 0.0;
#pragma unroll
        for (int i = 0; i < K; ++i)
          g += (rev ? bcoef(j, i) : ((i == j) ? -1.0 : 0.0)) * v[i];
        const int64_t dof = ta.cell_dofs ? (int64_t)ta.cell_dofs[fdof[it] + j] : fdof[it] + j;
        xc[dof] = fold[it][j] + g;
      }
    }
    if constexpr (NIC > 0)
    {
#pragma unroll
      for (int it = 0; it < NIE; ++it)
      {
        if (idof[it] < 0)
          continue;
        const int e = it * TILE_THREADS + threadIdx.x;
        const int cl = e / NIC, i = e - cl * NIC;
        xc[idof[it]] = iold[it] + packed_sum<K, NPK>(sSlots + (int64_t)cl * 3 * NPK, 3 * K + i);
      }
    }
    return;
  }

#pragma unroll
  for (int it = 0; it < NIT; ++it)
  {
    const int e = (it * TILE_THREADS + threadIdx.x) * VW;
    const int cl = e / NRT, i = e - cl * NRT;
    if (xi[it] >= 0)
    {
      const double* sl = sSlots + (int64_t)cl * 3 * NPK;
      if constexpr (VW == 2)
      {
        double2 t;
        t.x = xv[it][0] + packed_sum<K, NPK>(sl, i);
        t.y = xv[it][1] + packed_sum<K, NPK>(sl, i + 1);
        *reinterpret_cast<double2*>(x + xi[it]) = t;
      }
      else
        x[xi[it]] = xv[it][0] + packed_sum<K, NPK>(sl, i);
    }
  }
}

template <int K, int DEG, int MODE>
__global__ void __launch_bounds__(tile_threads_c(K), (K <= 2 ? 4 : 1)) k_se_patch_tiled(const SeArgs a0, const TileArgs ta)
{
  extern __shared__ __align__(16) double lds[];
  // XCD-aware order: workgroups are dealt round-robin to the 8 XCDs, tiles are numbered along the
  // bisection tree (neighbours in space are neighbours in index); give every XCD one contiguous
  // range of tiles so that the rim cells two tiles share are read through the same L2
  const int tile = ta.tile_first + xcd_remap(blockIdx.x, ta.ntiles);
  tile_stage<K, DEG, MODE>(a0, ta, tile, lds);
  tile_sweep_flush<K, DEG, MODE>(a0, ta, tile, lds);
}

// All right-hand sides of a call in ONE launch (se/solve_patch_semiexplt.hpp:1040-1075 loops the right-hand
// sides inside the patch): a workgroup per (tile, right-hand side); the workgroups of one tile are neighbours in
// the launch order of their XCD, so the tile's descriptors, geometry and tensors are read from HBM once and
// come from that XCD's L2 for the other right-hand sides.  A loop over the right-hand sides INSIDE the
// workgroup was built and measured first (tensors staged once per tile): the loop makes the compiler hoist
// lane predicates and table addresses out of it, 47 spilled registers, 0.565 ms for 4 right-hand sides at 1M
// triangles against 0.357 ms for four separate launches.  What the reference re-uses across the
// right-hand sides - the factorisation - is a handful of multipliers here; they are recomputed.
template <int K, int DEG, int MODE>
__global__ void __launch_bounds__(tile_threads_c(K), (K <= 2 ? 4 : 1))
k_se_patch_tiled_multi(const SeArgs a0, const TileArgs ta, const MultiRhs mr)
{
  extern __shared__ __align__(16) double lds[];
  const int pos = xcd_remap(blockIdx.x, ta.ntiles * mr.n);
  const int tile = ta.tile_first + pos / mr.n;
  const int r = pos - (pos / mr.n) * mr.n;
  SeArgs a = a0;
  a.rhs = mr.rhs0 + r;
  a.flux_dg = mr.g[r];
  a.rhs_dg = mr.f[r];
  a.out = mr.x[r];
  a.rhs_in = 0;
  a.rhs_out = 0;
  tile_stage<K, DEG, MODE>(a, ta, tile, lds);
  tile_sweep_flush<K, DEG, MODE>(a, ta, tile, lds);
}

template <int K, int DEG, int MODE>
static int launch_tiled_multi_kd(const SeArgs& a, const TileArgs& t, const MultiRhs& mr, hipStream_t stream)
{
  using Z = Sizes<K, DEG, 8>;
  const size_t lds_bytes
      = sizeof(double) * ((size_t)(K == 3 ? Z::NTAB_HALF : Z::NTAB) + (MODE ? (size_t)Z::NEV : 0) + (size_t)t.tc * 3 * (Z::NRT - K));
  if (lds_bytes > 160 * 1024 || t.tc < 1 || t.tc > tile_cells_max_c(K) || mr.n < 1 || mr.n > MULTI_RHS_MAX)
    return EQLB_ERR_UNSUPPORTED;
  auto kern = k_se_patch_tiled_multi<K, DEG, MODE>;
  if (lds_bytes > 64 * 1024)
  {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess)
      return EQLB_ERR_DEVICE;
  }
  if (t.ntiles == 0)
    return 0;
  hipLaunchKernelGGL(kern, dim3((unsigned)t.ntiles * (unsigned)mr.n), dim3(tile_threads_c(K)), lds_bytes, stream, a, t, mr);
  return (hipGetLastError() == hipSuccess) ? 0 : EQLB_ERR_DEVICE;
}

template <int K, int DEG, int MODE>
static int launch_tiled_kd(const SeArgs& a, const TileArgs& t, hipStream_t stream)
{
  using Z = Sizes<K, DEG, 8>;
  const size_t lds_bytes
      = sizeof(double) * ((size_t)(K == 3 ? Z::NTAB_HALF : Z::NTAB) + (MODE ? (size_t)Z::NEV : 0) + (size_t)t.tc * 3 * (Z::NRT - K));
  if (lds_bytes > 160 * 1024 || t.tc < 1 || t.tc > tile_cells_max_c(K))
    return EQLB_ERR_UNSUPPORTED;
  auto kern = k_se_patch_tiled<K, DEG, MODE>;
  if (lds_bytes > 64 * 1024)
  {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess)
      return EQLB_ERR_DEVICE;
  }
  if (t.ntiles == 0)
    return 0;
  hipLaunchKernelGGL(kern, dim3((unsigned)t.ntiles), dim3(tile_threads_c(K)), lds_bytes, stream, a, t);
  return (hipGetLastError() == hipSuccess) ? 0 : EQLB_ERR_DEVICE;
}

} // namespace eqlb
