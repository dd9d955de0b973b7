// Full 8-cell patches of RT_2 (SE mode, P1 data) on FOUR lanes, two consecutive ring cells per lane: the instance
// behind EQLB_PAIR_LANES of the tiled launch (k_se_patch_tiled_pair = k_se_patch_tiled<2, 1, 0> whose bin of P = 8
// hands the whole 16-patch wave-blocks of full patches to se_pair_body).  Lane l of a 4-lane group holds the ring
// cells 2 l and 2 l + 1: phases A, C, E of se_patch_body run once per held cell, the facet between the two cells is
// register arithmetic, only the facets between lanes go through DPP (quad_perm inside the group), and the chain is
// 4 lanes long (eqlb_pair_chain.h, which tools/pair_chain_emul.cpp runs on the host against the lane = cell
// arithmetic).  Rows go to the same packed LDS slots; the flush and every other instance are those of
// eqlb_se_kernels.hip, whose translation unit this one leaves alone.  launch_se_patch_tiled takes this kernel for
// handles with one right-hand side.
#include "eqlb_internal.h"

#if EQLB_PAIR_LANES
#include "eqlb_se_tile.h"
#include "eqlb_pair_chain.h"

namespace eqlb
{

// lane exchange of eqlb_pair_chain.h on the device: DPP quad_perm inside the 4-lane group of a patch
struct PairDpp
{
  using mask = bool;
  static __device__ __forceinline__ int sub()
  {
    int t = threadIdx.x; // (an opaque lane index is not needed here: 119 VGPRs either way)
    return t & 3;
  }
  static __device__ __forceinline__ double cst(double c) { return c; }
  static __device__ __forceinline__ double fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
  static __device__ __forceinline__ double rcp(double a) { return rcp_d(a); }
  // a pivot passes if it is positive and finite: one class test (+denormal | +normal) in place of the compare with
  // zero, which +inf passes as well
  static __device__ __forceinline__ bool pos(double a) { return __builtin_amdgcn_class(a, 0x180); }
  static __device__ __forceinline__ bool both(bool a, bool b) { return a && b; }
  static __device__ __forceinline__ double dn(double v) { return dpp_d<0x93>(v); }  // quad_perm [3,0,1,2]
  static __device__ __forceinline__ double up(double v) { return dpp_d<0x39>(v); }  // quad_perm [1,2,3,0]
  static __device__ __forceinline__ double dn2(double v) { return dpp_d<0x4E>(v); } // quad_perm [2,3,0,1]
  static __device__ __forceinline__ double b0(double v) { return dpp_d<0x00>(v); }  // quad_perm [0,0,0,0]
  static __device__ __forceinline__ double qsum(double v)
  {
    v += dpp_d<0xB1>(v); // quad_perm [1,0,3,2]
    v += dpp_d<0x4E>(v);
    return v;
  }
  static __device__ __forceinline__ double z0(double v) { return (sub() == 0) ? 0.0 : v; }
  static __device__ __forceinline__ double z01(double v) { return (sub() <= 1) ? 0.0 : v; }
  static __device__ __forceinline__ double z3(double v) { return (sub() == 3) ? 0.0 : v; }
  static __device__ __forceinline__ double one0(double v) { return (sub() == 0) ? 1.0 : v; }
  static __device__ __forceinline__ double only0(double v) { return (sub() == 0) ? v : 0.0; }
  static __device__ __forceinline__ double only3(double v) { return (sub() == 3) ? v : 0.0; }
  static __device__ __forceinline__ double sel0(double a, double b) { return (sub() == 0) ? a : b; }
};

// The two cells of a lane are independent until phase B and again in phase C.  Left alone, the compiler interleaves
// them, holds the table reads of both at once (phase C alone: 72 ds_read_b128) and keeps every value decoded from a
// descriptor alive to the end: 321 spilled registers.  pair_fence() passes a value through an empty volatile asm:
// what is computed from it cannot start before the fence, and fences keep their order, so a block of fences between
// two phases serialises them; a descriptor word that went through a fence is decoded again instead of held.
__device__ __forceinline__ void pair_fence(double& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void pair_fence(uint32_t& v) { asm volatile("" : "+v"(v)); }
// (an index that table addresses are formed from, behind a result: the reads wait for the result)
__device__ __forceinline__ void pair_fence(int& idx, double& r) { asm volatile("" : "+v"(idx), "+v"(r)); }
template <int N>
__device__ __forceinline__ void pair_fence(double (&v)[N])
{
#pragma unroll
  for (int i = 0; i < N; ++i)
    pair_fence(v[i]);
}

// the fields of a slot descriptor and what follows from them; bit 31 of the word (the 1-based position of the cell in
// its tile, at most 491, sits in bits 8 and up) carries the orientation of the cell, det J < 0, from phase A on: no
// register for the sign
constexpr uint32_t PAIR_NEG = 1u << 31;
struct PairDesc
{
  int fm, fp, ln, ci;
  uint32_t loc;
  double rho_m, rho_p, pf_m, pf_p, sgn;
  __device__ __forceinline__ PairDesc(const uint32_t info)
  {
    sgn = (info & PAIR_NEG) ? -1.0 : 1.0;
    fm = (info >> INFO_FM_SHIFT) & 3;
    fp = (info >> INFO_FP_SHIFT) & 3;
    ln = (info >> INFO_LN_SHIFT) & 3;
    const bool rev_m = (info & INFO_REV_M) != 0, rev_p = (info & INFO_REV_P) != 0;
    ci = combo_index(fm, fp, rev_m);
    rho_m = rev_m ? 1.0 : 0.0;
    rho_p = rev_p ? 1.0 : 0.0;
    loc = (info & ~PAIR_NEG) >> INFO_LOCAL_SHIFT;
    pf_m = (fm == 1) ? sgn : -sgn; // facet 1 measures the outward flux
    pf_p = (fp == 1) ? sgn : -sgn;
  }
};

template <int K, int DEG>
__device__ __forceinline__ void se_pair_body(const SeArgs& a, const int64_t slot_base, const int lane, double* lds,
                                             double* tile_slots)
{
  static_assert(K == 2 && DEG == 1, "the pair-lane instance is written for RT_2 with P1 data");
  using Z = Sizes<2, 1, 8>;
  using X = PairDpp;
  constexpr int ND = Z::ND, NQ = Z::NQ, NH = Z::NH, NCOL = Z::NCOL, NTES = Z::NTES, NCOLS = Z::NCOLS;
  constexpr int NPK = Z::NRT - K;
  static_assert(ND == 3 && NQ == 3 && NH == 3 && NCOL == 6 && NTES == 6 && NCOLS == 6 && NPK == 6, "RT_2 / P1 sizes");
  const double* sF = lds;
  const double* sH = sF + Z::NF;
  const double* sTE = sH + Z::NHT + Z::NDT;
  const double* sWQ = sTE + Z::NTET;

  // descriptors of the two cells: consecutive slots of the lane-contiguous SoA, one 8-byte load each (the slot lists
  // of a tile start on multiples of 64 slots); then J, G, f of both cells in one batch
  // (the lane offset formed here, behind an empty asm: otherwise the loop over the wave-blocks carries the two
  // addresses as 64-bit induction variables in registers this body needs)
  int l2 = 2 * lane;
  asm volatile("" : "+v"(l2));
  const int64_t slot = a.slot_offset + slot_base + l2;
  const int2 cells = *reinterpret_cast<const int2*>(a.slot_cell + slot);
  const uint2 infos = *reinterpret_cast<const uint2*>(a.slot_info + slot);
  uint32_t info[2] = {infos.x, infos.y};
  double Jc[2][4], gx[2][ND], gy[2][ND], fdat[2][ND];
#pragma unroll
  for (int c = 0; c < 2; ++c)
  {
    const int32_t cell = c ? cells.y : cells.x;
    const double2* Jp = reinterpret_cast<const double2*>(a.cellJ + 4 * (int64_t)cell);
    const double2* gp_ = reinterpret_cast<const double2*>(a.flux_dg + ((int64_t)a.rhs_in * a.ncells + cell) * (ND * 2));
    const double* fp_ = a.rhs_dg + ((int64_t)a.rhs_in * a.ncells + cell) * ND;
    const double2 j0 = Jp[0], j1 = Jp[1];
#pragma unroll
    for (int i = 0; i < ND; ++i)
    {
      const double2 g2 = gp_[i];
      gx[c][i] = g2.x;
      gy[c][i] = g2.y;
    }
#pragma unroll
    for (int i = 0; i < ND; ++i)
      fdat[c][i] = fp_[i];
    Jc[c][0] = j0.x;
    Jc[c][1] = j0.y;
    Jc[c][2] = j1.x;
    Jc[c][3] = j1.y;
  }

  // ---- phase A per cell (se_patch_body, MODE 0, P1 data); kept: the metric g = J^T J / |det J| ----
  double gm[2][K], gpv[2][K], Rq[2][NQ], met[2][3];
#pragma unroll
  for (int c = 0; c < 2; ++c)
  {
    if (c == 1)
    {
      pair_fence(gm[0]);
      pair_fence(gpv[0]);
      pair_fence(Rq[0]);
      pair_fence(met[0]);
      pair_fence(Jc[1]);
      pair_fence(gx[1]);
      pair_fence(gy[1]);
      pair_fence(fdat[1]);
      pair_fence(info[1]);
    }
    // (first everything that needs no table - the loaded data shrink to 9 doubles per cell and the metric - then the
    // table reads in batches, each behind the arithmetic of the one before)
    const int fm = (info[c] >> INFO_FM_SHIFT) & 3, fp = (info[c] >> INFO_FP_SHIFT) & 3;
    int ln = (info[c] >> INFO_LN_SHIFT) & 3;
    double gnm[ND], gnp[ND], wv[ND], pf_m, pf_p;
    {
      const double J00 = Jc[c][0], J01 = Jc[c][1], J10 = Jc[c][2], J11 = Jc[c][3];
      const double detJ = J00 * J11 - J01 * J10;
      info[c] |= (detJ > 0.0) ? 0u : PAIR_NEG;
      const double sg = (detJ > 0.0) ? 1.0 : -1.0;
      pf_m = (fm == 1) ? sg : -sg; // facet 1 measures the outward flux
      pf_p = (fp == 1) ? sg : -sg;
      const double ia = rcp_d(fabs(detJ));
      met[c][0] = (J00 * J00 + J10 * J10) * ia;
      met[c][1] = (J00 * J01 + J10 * J11) * ia;
      met[c][2] = (J01 * J01 + J11 * J11) * ia;
      const double a00 = J11, a01 = -J01, a10 = -J10, a11 = J00;
      const double nmx = (fm == 2) ? 0.0 : -1.0, nmy = (fm == 0) ? -1.0 : ((fm == 1) ? 0.0 : 1.0);
      const double npx = (fp == 2) ? 0.0 : -1.0, npy = (fp == 0) ? -1.0 : ((fp == 1) ? 0.0 : 1.0);
      const double num0 = a00 * nmx + a10 * nmy, num1 = a01 * nmx + a11 * nmy;
      const double nup0 = a00 * npx + a10 * npy, nup1 = a01 * npx + a11 * npy;
      double dvg = 0.0;
#pragma unroll
      for (int i = 0; i < ND; ++i)
      {
        const double g2x = gx[c][i], g2y = gy[c][i];
        gnm[i] = g2x * num0 + g2y * num1;
        gnp[i] = g2x * nup0 + g2y * nup1;
        const double gh0 = a00 * g2x + a01 * g2y;
        const double gh1 = a10 * g2x + a11 * g2y;
        wv[i] = detJ * fdat[c][i];
        if (i == 0)
          dvg = -(gh0 + gh1);
        else if (i == 1)
          dvg += gh0;
        else
          dvg += gh1;
      }
#pragma unroll
      for (int i = 0; i < ND; ++i)
        wv[i] -= dvg;
    }
#pragma unroll
    for (int j = 0; j < K; ++j)
      gm[c][j] = gpv[c][j] = 0.0;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      Rq[c][q] = 0.0;
    pair_fence(ln, wv[ND - 1]);
    pair_fence(gnm);
    pair_fence(gnp);
    pair_fence(met[c]);
    {
      const double* tF_m = row16<true>(sF + (fm * 3 + ln) * ND * K);
      const double* tF_p = row16<true>(sF + (fp * 3 + ln) * ND * K);
#pragma unroll
      for (int i = 0; i < ND; ++i)
      {
        double rm[K], rp[K];
        ldrow16<K>(tF_m + i * K, rm);
        ldrow16<K>(tF_p + i * K, rp);
#pragma unroll
        for (int j = 0; j < K; ++j)
        {
          gm[c][j] += rm[j] * gnm[i];
          gpv[c][j] += rp[j] * gnp[i];
        }
      }
#pragma unroll
      for (int j = 0; j < K; ++j)
      {
        gm[c][j] *= pf_m;
        gpv[c][j] *= pf_p;
      }
    }
    pair_fence(gm[c]);
    pair_fence(ln, gpv[c][K - 1]);
    {
      const double* tH = row16<true>(sH + ln * Z::HROW);
      double rH[Z::HROW];
      ldrow16<Z::HROW>(tH, rH);
#pragma unroll
      for (int i = 0; i < ND; ++i)
#pragma unroll
        for (int q = 0; q < NQ; ++q)
          Rq[c][q] += wv[i] * rH[i * NQ + q];
    }
  }

  // ---- phase B: the facet between the two cells from registers, the facets between lanes by DPP ----
  double mu_m[2][K], mu_p0[2];
  {
    const double rho_m[2] = {(info[0] & INFO_REV_M) ? 1.0 : 0.0, (info[1] & INFO_REV_M) ? 1.0 : 0.0};
    const double rho_p[2] = {(info[0] & INFO_REV_P) ? 1.0 : 0.0, (info[1] & INFO_REV_P) ? 1.0 : 0.0};
    const double sr0[2] = {(info[0] & PAIR_NEG) ? -Rq[0][0] : Rq[0][0], (info[1] & PAIR_NEG) ? -Rq[1][0] : Rq[1][0]};
    eqlb_pair::pair_phase_b<double, X>(gm, gpv, rho_m, rho_p, sr0, mu_m, mu_p0);
  }

  // ---- phase C per cell: element matrix and load from the reduced reference tensors ----
  double te[2][NTES], le[2][NH];
#pragma unroll
  for (int c = 0; c < 2; ++c)
  {
    if (c == 1)
    {
      pair_fence(te[0]);
      pair_fence(le[0]);
      pair_fence(met[1]);
      pair_fence(mu_m[1]);
      pair_fence(mu_p0[1]);
      pair_fence(Rq[1]);
    }
    pair_fence(info[c]);
    const PairDesc p(info[c]);
    const double g0 = met[c][0], g1 = met[c][1], g2 = met[c][2];
    // (the 36 table reads of a cell in four batches, each behind the arithmetic of the one before: issued at once - and
    // above phase B, since their addresses need the descriptor only - they fill 144 registers)
    int ci = p.ci;
    pair_fence(ci, mu_p0[c]);
    const double* tep = row16<true>(sTE + ci * 3 * NTES);
#pragma unroll
    for (int e2 = 0; e2 < NTES / 2; ++e2)
    {
      const double2 t0 = reinterpret_cast<const double2*>(tep)[e2];
      const double2 t1 = reinterpret_cast<const double2*>(tep + NTES)[e2];
      const double2 t2 = reinterpret_cast<const double2*>(tep + 2 * NTES)[e2];
      te[c][2 * e2] = g0 * t0.x + g1 * t1.x + g2 * t2.x;
      te[c][2 * e2 + 1] = g0 * t0.y + g1 * t1.y + g2 * t2.y;
    }
    pair_fence(te[c]); // (all of them: a value no fence asks for is computed late, and its table rows wait with it)
    const double full[NCOL] = {mu_m[c][0], mu_m[c][1], mu_p0[c], 0.0, p.sgn * Rq[c][1], p.sgn * Rq[c][2]};
#pragma unroll
    for (int h = 0; h < NH; ++h)
    {
      double sx[3];
#pragma unroll
      for (int x = 0; x < 3; ++x)
      {
        // (the load tensor in batches of one metric row, 3 reads of 16 bytes: all 9 at once spill 86 registers)
        pair_fence(ci, (x > 0) ? sx[x - 1] : ((h == 0) ? te[c][NTES - 1] : le[c][h - 1]));
        const double* wq = row16<true>(sWQ + ci * 3 * NH * NCOLS + (x * NH + h) * NCOLS);
        double s_ = 0.0;
#pragma unroll
        for (int c2 = 0; c2 < NCOLS / 2; ++c2)
        {
          const double2 w = reinterpret_cast<const double2*>(wq)[c2];
          s_ = __builtin_fma(w.x, full[2 * c2], s_);
          if (2 * c2 + 1 != K + 1) // (column of mu_p[1]: zero on an interior patch)
            s_ = __builtin_fma(w.y, full[2 * c2 + 1], s_);
        }
        sx[x] = s_;
      }
      le[c][h] = -(g0 * sx[0] + g1 * sx[1] + g2 * sx[2]);
    }
    // the divergence DOFs of the row do not wait for the solve
    if (p.loc != 0u)
    {
      double* o = tile_slots + ((int64_t)(p.loc - 1) * 3 + p.ln) * NPK;
      o[2 * K] = Rq[c][1];
      o[2 * K + 1] = Rq[c][2];
    }
  }

  // ---- reduced system: border [d ; x_0] and the chain over 4 lanes ----
  double d, xe, xo, xn;
  bool posdef;
  eqlb_pair::pair_chain<double, X>(te, le, d, xe, xo, xn, posdef);
  if (!posdef)
    atomicOr(a.status, 1);

  // ---- phase E per cell: back-map to RT coefficients, rows to the LDS slots of the owned cells ----
#pragma unroll
  for (int c = 0; c < 2; ++c)
  {
    pair_fence(info[c]);
    const PairDesc p(info[c]);
    if (p.loc == 0u)
      continue;
    const double um = c ? xo : xe, up = c ? xn : xo;
    double u0, u1;
    eqlb_pair::rev2<double, X>(d, um, p.rho_m, u0, u1);
    const double ym[K] = {mu_m[c][0] - u0, mu_m[c][1] - u1};
    const double yp[K] = {mu_p0[c] + d, up};
    double* o = tile_slots + ((int64_t)(p.loc - 1) * 3 + p.ln) * NPK;
    const int pm = p.fm - ((p.fm > p.ln) ? 1 : 0), pp = p.fp - ((p.fp > p.ln) ? 1 : 0);
#pragma unroll
    for (int j = 0; j < K; ++j)
    {
      o[pm * K + j] = p.pf_m * ym[j];
      o[pp * K + j] = p.pf_p * yp[j];
    }
  }
}

__global__ void __launch_bounds__(tile_threads_c(2), 4) k_se_patch_tiled_pair(const SeArgs a0, const TileArgs ta)
{
  extern __shared__ __align__(16) double lds[];
  const int tile = ta.tile_first + xcd_remap(blockIdx.x, ta.ntiles);
  tile_stage<2, 1, 0>(a0, ta, tile, lds);
  tile_sweep_flush<2, 1, 0, true>(a0, ta, tile, lds);
}

bool pair_lanes_built() { return true; }

int launch_se_patch_tiled_pair(const SeArgs& a, const TileArgs& t, hipStream_t stream)
{
  using Z = Sizes<2, 1, 8>;
  const size_t lds_bytes = sizeof(double) * ((size_t)Z::NTAB + (size_t)t.tc * 3 * (Z::NRT - 2));
  if (lds_bytes > 160 * 1024 || t.tc < 1 || t.tc > tile_cells_max_c(2))
    return EQLB_ERR_UNSUPPORTED;
  if (lds_bytes > 64 * 1024)
  {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_se_patch_tiled_pair),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess)
      return EQLB_ERR_DEVICE;
  }
  if (t.ntiles == 0)
    return 0;
  hipLaunchKernelGGL(k_se_patch_tiled_pair, dim3((unsigned)t.ntiles), dim3(tile_threads_c(2)), lds_bytes, stream, a, t);
  return (hipGetLastError() == hipSuccess) ? 0 : EQLB_ERR_DEVICE;
}

} // namespace eqlb
#else
namespace eqlb
{
bool pair_lanes_built() { return false; }
int launch_se_patch_tiled_pair(const SeArgs&, const TileArgs&, hipStream_t) { return EQLB_ERR_UNSUPPORTED; }
} // namespace eqlb
#endif
