// What the three weak-symmetry kernels share: k_se_weaksym (eqlb_se_weaksym.hip: dense tiles in LDS, the small bins),
// k_se_weaksym_banded (eqlb_se_weaksym_banded.hip: one patch per wave, RT_4 with 9 ... 64 facets and RT_3 with
// 33 ... 64) and k_se_weaksym_large (eqlb_se_weaksym_large.hip: one workgroup per patch, more than 63 cells).
//
// The contract of all three.  They run after the row-wise flux kernels: the slot buffer a.out then holds the
// patch-local stress rows sigma_a, one slot row per (cell, vertex) and right-hand side.  Per patch they solve
//   [A 0 B0; 0 A B1; B0^T B1^T 0 (+ mean-value row)] [u0; u1; gamma] = [0; 0; Lc]
//   B0(i,j) = int (Phi_i)_y psi_j,  B1(i,j) = -int (Phi_i)_x psi_j,  Lc(j) = -int psi_j (s01 - s10)
// over the patch-wise H(div=0) functions Phi_i and the patch P1 functions psi_j (impose_weak_symmetry,
// se/solve_patch_weaksym.hpp:59-233, with assemble_stressminimiser, se/assembly.hpp:292-472), quadrature-free with the
// tensors TE, V, VQ of tools/gen_tables.py, through the Schur complement C = M - sum_k Y_k^T Y_k, Y_k = L_k^-1 B_k,
// A_k = L_k L_k^T; with flux BCs on a stress row the masked A_k and B_k of that row.  The Schur system is eliminated
// with row pivoting and the rank-revealing threshold EQLB_WS_PIVOT_RTOL: the multiplier of a column without pivot is
// 0.  u_k = -A_k^-1 B_k gamma is added to the slot rows of right-hand sides 0 and 1 in place.  Two-cell patches of a
// group have no step of their own (PFLAG_WS_SKIP), the internal patch of a group works on its own rows plus those of
// the group's two-cell patches (PFLAG_WS_GROUP), one pass per level of overlapping groups (a.ws_level).  A pivot
// of a Cholesky factor that is not positive sets bit 2 of a.status (in the banded and the large kernel a pivot, an
// entry of the Schur system or a multiplier that is not finite does so too).
//
// Shared here: the patch flags (WsPatch of eqlb_se_weaksym_numbering.h, decoded by ws_patch), the cell (WsCell: decode,
// J, metric, element entries, load, points, write-back), the serial back substitution of the Schur system and the
// launch helper for more than 64 KB of LDS; in the numbering header the integer rules.  NOT shared, because each
// kernel spreads them over its lanes in its own way: the storage of the factor, the factorisation, the substitutions
// of Y, the accumulation of the Schur matrix and the pivot search.
#pragma once

#include "eqlb_device_common.h"
#include "eqlb_se_weaksym_numbering.h"

namespace eqlb
{

// flags of right-hand sides 0 and 1 (bits as in k_se_patch) and the cell count
__device__ __forceinline__ WsPatch ws_patch(uint8_t flag0, uint8_t flag1, int n)
{
  return WsPatch((flag0 & PFLAG_INTERIOR) != 0, n, (flag0 & PFLAG_BC0) != 0, (flag0 & PFLAG_BCN) != 0,
                 (flag1 & PFLAG_BC0) != 0, (flag1 & PFLAG_BCN) != 0);
}

// Cell i of the fan of a patch, read from its lane slot.  An inactive lane (no cell) gets the unit cell with no area
// (ia = 0): its entries are never added.
template <int K>
struct WsCell
{
  using Z = Sizes<K, K - 1, 64>; // (only what does not depend on the bin)
  using N = WsNumbering<K>;
  static constexpr int KB = N::KB, NADD = N::NADD, NH = N::NH, NRT = Z::NRT;
  static_assert(KB == Z::KB && NADD == Z::NADD && NH == Z::NH, "the numbering header counts as Sizes does");

  int32_t cell;
  uint32_t info;
  int fm, fp, ln, ci;
  bool rev_m;
  double J00, J01, J10, J11, detJ, sgn, pf_m, pf_p, g0, g1, g2; // (scalars: see WsPatch)
  int pj0, pj1, pj2;
  const double *te, *vq; // the rows of the cell's facet combination in the tensors TE and VQ

  // te_table, vq_table: the tensors TE and VQ (Z::OFF_TE, Z::OFF_VQ of the tables), in LDS or in global memory.  (The
  // rows are taken here, once: formed at every entry they cost k_se_weaksym_banded<4, P> 1000 instructions.)
  __device__ __forceinline__ WsCell(const SeArgs& a, const double* te_table, const double* vq_table, int64_t slot,
                                    bool active, const WsPatch& p, int i)
  {
    cell = active ? a.slot_cell[slot] : 0;
    info = active ? a.slot_info[slot] : 0u;
    fm = (info >> INFO_FM_SHIFT) & 3;
    fp = (info >> INFO_FP_SHIFT) & 3;
    ln = (info >> INFO_LN_SHIFT) & 3;
    rev_m = (info & INFO_REV_M) != 0;
    ci = active ? combo_index(fm, fp, rev_m) : 0;
    te = te_table + ci * 3 * Z::NTES;
    vq = vq_table + ci * 2 * NH * 3;
    J00 = J11 = 1.0;
    J01 = J10 = 0.0;
    if (active)
    {
      const double2* Jp = reinterpret_cast<const double2*>(a.cellJ + 4 * (int64_t)cell);
      const double2 j0 = Jp[0], j1 = Jp[1];
      J00 = j0.x;
      J01 = j0.y;
      J10 = j1.x;
      J11 = j1.y;
    }
    detJ = J00 * J11 - J01 * J10;
    sgn = (detJ > 0.0) ? 1.0 : -1.0;
    pf_m = (fm == 1) ? sgn : -sgn;
    pf_p = (fp == 1) ? sgn : -sgn;
    const double ia = active ? 1.0 / fabs(detJ) : 0.0;
    g0 = (J00 * J00 + J10 * J10) * ia;
    g1 = (J00 * J01 + J10 * J11) * ia;
    g2 = (J01 * J01 + J11 * J11) * ia;
    int pts[3];
    ws_points(p, i, fm, fp, ln, pts);
    pj0 = pts[0];
    pj1 = pts[1];
    pj2 = pts[2];
  }
  // multiplier DOF of local vertex j
  __device__ __forceinline__ int pj(int j) const { return (j == 0) ? pj0 : ((j == 1) ? pj1 : pj2); }

  // Te(h, g) = int Phi_h . Phi_g
  __device__ __forceinline__ double Te(int h, int g) const
  {
    const int e = (h >= g) ? h * (h + 1) / 2 + g : g * (g + 1) / 2 + h;
    return g0 * te[e] + g1 * te[Z::NTES + e] + g2 * te[2 * Z::NTES + e];
  }
  // Be(k, h, j): k = 0: int (Phi_h)_y psi_j ; k = 1: -int (Phi_h)_x psi_j
  __device__ __forceinline__ double Be(int k, int h, int j) const
  {
    const double v0 = vq[h * 3 + j], v1 = vq[(NH + h) * 3 + j];
    return (k == 0) ? (J10 * v0 + J11 * v1) : -(J00 * v0 + J01 * v1);
  }
  // |T| / 6 = int psi_j: the coupling with the mean-value multiplier
  __device__ __forceinline__ double Ce() const { return fabs(detJ) / 6.0; }
  // the patch-local stress row of right-hand side k in the slots
  __device__ __forceinline__ double* row(double* out, int32_t ncells, int k) const
  {
    return out + (((int64_t)k * ncells + cell) * 3 + ln) * NRT;
  }
  // Lce[j] -= int psi_j (s01 - s10) of the cell's rows; grouped patches (modified_patch,
  // se/solve_patch_weaksym.hpp:100-131): the stress accumulated by the group so far = own rows + the rows of the
  // group's two-cell patches on this cell.  sV: the tensor V (Z::OFF_V).  UNROLL: the loop over the row is unrolled
  template <bool UNROLL>
  __device__ __forceinline__ void load(double* out, int32_t ncells, bool grouped, const double* sV, double Lce[3]) const
  {
    const double *r0 = row(out, ncells, 0), *r1 = row(out, ncells, 1);
    const uint32_t grows = grouped ? ((info >> INFO_GROUPROW_SHIFT) & 7u) : 0u;
    auto term = [&](int i) {
      double c0 = r0[i], c1 = r1[i];
      if (grows)
      {
#pragma unroll
        for (int v = 0; v < 3; ++v)
          if (grows & (1u << v))
          {
            c0 += out[(((int64_t)0 * ncells + cell) * 3 + v) * NRT + i];
            c1 += out[(((int64_t)1 * ncells + cell) * 3 + v) * NRT + i];
          }
      }
      const double w0 = c0 * J10 - c1 * J00, w1 = c0 * J11 - c1 * J01;
#pragma unroll
      for (int j = 0; j < 3; ++j)
        Lce[j] -= sgn * (w0 * sV[(j * NRT + i) * 2] + w1 * sV[(j * NRT + i) * 2 + 1]);
    };
    if constexpr (UNROLL)
    {
#pragma unroll
      for (int i = 0; i < NRT; ++i)
        term(i);
    }
    else
    {
#pragma nounroll
      for (int i = 0; i < NRT; ++i)
        term(i);
    }
  }
  // back-map of the local solution ul [d | um | up | ua] and add to the slot row o of its right-hand side
  // (se/solve_patch_weaksym.hpp:189-232)
  __device__ __forceinline__ void add_correction(const double ul[NH], double* o) const
  {
#pragma unroll
    for (int j = 0; j < K; ++j)
    {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < K; ++c)
        s -= (rev_m ? bcoef(j, c) : ((j == c) ? 1.0 : 0.0)) * ul[c];
      const double yp = (j == 0) ? ul[0] : ul[KB + j];
      o[fm * K + j] += pf_m * s;
      o[fp * K + j] += pf_p * yp;
    }
#pragma unroll
    for (int q = 0; q < NADD; ++q)
      o[3 * K + Z::NDIV + q] += sgn * ul[1 + 2 * KB + q];
  }
};

// Back substitution of the eliminated Schur system [C | R] (rows of ld entries) over the pivot columns, right to left,
// by one thread: pcol[c] is the row that eliminated column c, or negative: no pivot, multiplier 0.  A multiplier that
// is not finite sets *status where status is given.
template <class LD, class PC>
__device__ __forceinline__ void ws_back_substitute(const double* C, LD ld, const double* R, const PC* pcol, int dim_c,
                                                   double* gamma, int* status)
{
  for (int c = dim_c - 1; c >= 0; --c)
  {
    if (pcol[c] < 0)
    {
      gamma[c] = 0.0;
      continue;
    }
    const LD r = pcol[c];
    double t = R[r];
    for (int j = c + 1; j < dim_c; ++j)
      t -= C[r * ld + j] * gamma[j];
    gamma[c] = t / C[r * ld + c];
    if (status && !isfinite(gamma[c]))
      *status = 1;
  }
}

// a kernel with more than 64 KB of dynamic LDS has to be told so before its launch
template <class Kernel>
inline bool ws_allow_lds(Kernel kern, size_t lds_bytes)
{
  return lds_bytes <= 64 * 1024
         || hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds_bytes)
                == hipSuccess;
}

} // namespace eqlb
