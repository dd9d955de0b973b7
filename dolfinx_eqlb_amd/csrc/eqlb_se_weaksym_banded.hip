// Weak symmetry of equilibrated stresses for the large bins: RT_4 with patches of 9 ... 64 facets and RT_3
// with 33 ... 64 facets.  Same contract and same solution as k_se_weaksym (eqlb_se_weaksym.hip) - input
// SeArgs, corrections added to the slot rows of RHS 0 and 1 in place, grouped patches, one pass per
// level of overlapping groups, the same rank-revealing LU of the Schur system - but the LDS grows
// linearly with the patch instead of quadratically, so these bins fit a workgroup.
//
// One patch per wave (64 lanes; lane i <-> cell T_{i+1}).  The unknowns of the patch are ordered as a
// banded chain plus a border:
//   chain   [a_0 | x_1 | a_1 | x_2 | ... ]   a_s: the NADD cell-bubble unknowns of cell s, x_f: the KB
//                                           unknowns of facet f >= 1 (boundary patches end with x_n)
//   border  [d | x_0]                        the patch-node unknown and facet 0 (closes the ring of
//                                           interior patches)
// A cell couples [x_s | a_s | x_{s+1}] and the border only, so the chain has half bandwidth
// BW = 2 KB + NADD - 1 and the Cholesky factor L = [Lc 0; Lb Lbb] keeps that profile: Lc is stored as
// a band, Lb / Lbb as NBD = 1 + KB dense rows.  B_k (H(div=0) functions against the patch P1
// functions) has at most four entries per row - the patch node and the ring points of the cells on
// either side - except the dense row of d; it is stored in that compressed form.
//   S = sum_k B_k^T A_k^-1 B_k = sum_k Y_k^T Y_k,  Y_k = L_k^-1 B_k
// is accumulated without storing Y: every lane runs the forward substitution of its columns of B_k
// along the chain (a sliding window of BW values + NBD border sums in registers), the rows of Y go
// through a buffer of RCH rows and are folded into S chunk by chunk.  S (at most 67^2 doubles) is
// eliminated in LDS by Gauss-Jordan with row pivoting and the rank-revealing threshold of the dense
// kernel, u_k = -A_k^-1 (B_k gamma) is one forward and one back substitution per stress row.
// With flux BCs the two rows have masked matrices: their factors are computed one after the other in the
// same buffer (A_1 for Y_1 and u_1, A_0 again for u_0).
#include "eqlb_device_common.h"
#include "eqlb_tables_gen.h"

namespace eqlb
{

template <int K, int P>
struct WsBand
{
  using Z = Sizes<K, K - 1, P>;
  static constexpr int KB = Z::KB, NADD = Z::NADD, NH = Z::NH, NRT = Z::NRT;
  static constexpr int DIMMAX = Z::DIMMAX;     // H(div=0) unknowns of a patch
  static constexpr int NBD = 1 + KB;           // border: d, x_0
  static constexpr int NCHMAX = DIMMAX - NBD;  // chain
  static constexpr int BW = 2 * KB + NADD - 1; // half bandwidth of the chain
  static constexpr int NPMAX = P + 2;          // patch nodes (multiplier DOFs)
  static constexpr int DCMAX = NPMAX + 1;      // + mean-value multiplier
  static constexpr int LDY = 2 * NPMAX;        // row of the Y buffer: Y_0 | Y_1
  static constexpr int RCH = 8;                // rows of Y per chunk
  static constexpr int NCT = (LDY + 63) / 64;  // columns of B_0 | B_1 per lane
  // LDS (doubles): band [NCHMAX][BW+1] | border [NBD][DIMMAX] | 1/L_ii [DIMMAX] | Bv [2][DIMMAX][4] |
  // Bd [2][NPMAX] | C [DCMAX][DCMAX] | R [DCMAX] | gamma [DCMAX] | Y buffer [RCH][LDY] (later w [2][DIMMAX]) |
  // ints: Bp [DIMMAX] (ring points of the B slots 1..3, one byte each) | pivot rows [DCMAX]
  static constexpr int OFF_BORD = NCHMAX * (BW + 1), OFF_DINV = OFF_BORD + NBD * DIMMAX;
  static constexpr int FACTOR = OFF_DINV + DIMMAX;
  static constexpr int OFF_BV = FACTOR, OFF_BD = OFF_BV + 2 * DIMMAX * 4, OFF_C = OFF_BD + 2 * NPMAX;
  static constexpr int OFF_R = OFF_C + DCMAX * DCMAX, OFF_G = OFF_R + DCMAX, OFF_Y = OFF_G + DCMAX;
  static constexpr int NYB = (RCH * LDY > 2 * DIMMAX) ? RCH * LDY : 2 * DIMMAX;
  static constexpr int OFF_INT = OFF_Y + NYB;
  static constexpr int NINT = DIMMAX + DCMAX;
  static constexpr int lds_doubles() { return OFF_INT + (NINT + 1) / 2; }
  static_assert(P <= 64 && NCT <= 3, "one patch per wave");
};

template <int K, int P>
__global__ void __launch_bounds__(64) k_se_weaksym_banded(const SeArgs a)
{
  using W = WsBand<K, P>;
  using Z = typename W::Z;
  constexpr int KB = W::KB, NADD = W::NADD, NH = W::NH, NRT = W::NRT, NBD = W::NBD, BW = W::BW;
  constexpr int DIMMAX = W::DIMMAX, NPMAX = W::NPMAX, DCMAX = W::DCMAX, LDY = W::LDY, RCH = W::RCH;
  constexpr int NCT = W::NCT, LDB = BW + 1;

  const int64_t patch_local = blockIdx.x;
  const int64_t patch = a.patch_offset + patch_local;
  // two-cell patches of a group have no weak-symmetry step of their own; patches of another level of
  // overlapping groups are left to that level's pass (uniform over the block: one patch per wave)
  const uint8_t flag0 = a.pflag[patch];
  if ((flag0 & PFLAG_WS_SKIP) != 0 || (int)((flag0 >> PFLAG_WS_LEVEL_SHIFT) & 3) != a.ws_level)
    return;

  extern __shared__ double lds[];
  double* band = lds;
  double* bord = lds + W::OFF_BORD;
  double* dinv = lds + W::OFF_DINV;
  double* Bv = lds + W::OFF_BV;
  double* Bd = lds + W::OFF_BD;
  double* Cg = lds + W::OFF_C;
  double* Rg = lds + W::OFF_R;
  double* Gg = lds + W::OFF_G;
  double* Yb = lds + W::OFF_Y;
  int* Bp = reinterpret_cast<int*>(lds + W::OFF_INT);
  int* pcol = Bp + DIMMAX;

  const int sub = threadIdx.x;
  const int64_t slot = a.slot_offset + patch_local * P + sub;
  const bool grouped = (flag0 & PFLAG_WS_GROUP) != 0;
  const int n = (int)a.pn[patch];
  const bool active = sub < n;
  const int32_t cell = active ? a.slot_cell[slot] : 0;
  const uint32_t info = active ? a.slot_info[slot] : 0u;
  const int fm = (info >> INFO_FM_SHIFT) & 3, fp = (info >> INFO_FP_SHIFT) & 3;
  const int ln = (info >> INFO_LN_SHIFT) & 3;
  const bool rev_m = (info & INFO_REV_M) != 0;
  const int ci = active ? combo_index(fm, fp, rev_m) : 0;

  double J[2][2] = {{1.0, 0.0}, {0.0, 1.0}};
  if (active)
  {
    const double2* Jp = reinterpret_cast<const double2*>(a.cellJ + 4 * (int64_t)cell);
    const double2 j0 = Jp[0], j1 = Jp[1];
    J[0][0] = j0.x;
    J[0][1] = j0.y;
    J[1][0] = j1.x;
    J[1][1] = j1.y;
  }
  const double detJ = J[0][0] * J[1][1] - J[0][1] * J[1][0];
  const double sgn = (detJ > 0.0) ? 1.0 : -1.0;
  const double pf_m = (fm == 1) ? sgn : -sgn, pf_p = (fp == 1) ? sgn : -sgn;

  const uint8_t flag1 = a.pflag[a.npatch_total + patch];
  const bool interior = (flag0 & PFLAG_INTERIOR) != 0;
  const int nf = interior ? n : n + 1;
  const int fi_p = interior ? ((sub + 1 < n) ? sub + 1 : 0) : sub + 1;
  const int dim = 1 + KB * nf + NADD * n;
  const int nch = dim - NBD;
  const int npnt = nf + 1;
  // flux BCs of the two rows (bits as in k_se_patch); PatchData::reinitialisation :175-206
  const bool bc0[2] = {(flag0 & PFLAG_BC0) != 0, (flag1 & PFLAG_BC0) != 0};
  const bool bcn[2] = {(flag0 & PFLAG_BCN) != 0, (flag1 & PFLAG_BCN) != 0};
  const bool requires_bcs = bc0[0] || bcn[0] || bc0[1] || bcn[1];
  // mean-value multiplier unless some row has a primal-Dirichlet end (type essnt_primal or mixed)
  const bool row_dual[2] = {!interior && bc0[0] && bcn[0], !interior && bc0[1] && bcn[1]};
  const bool meanvalue = interior || (row_dual[0] && row_dual[1]);
  const int dim_c = meanvalue ? npnt + 1 : npnt;

  // ---- element quantities (the tables are read from global memory: they would cost the LDS of a patch) ----
  const double ia = active ? 1.0 / fabs(detJ) : 0.0;
  const double g0 = (J[0][0] * J[0][0] + J[1][0] * J[1][0]) * ia,
               g1 = (J[0][0] * J[0][1] + J[1][0] * J[1][1]) * ia,
               g2 = (J[0][1] * J[0][1] + J[1][1] * J[1][1]) * ia;
  const double* te = a.tables + Z::OFF_TE + ci * 3 * Z::NTES;
  auto Te = [&](int h, int g) {
    const int e = (h >= g) ? h * (h + 1) / 2 + g : g * (g + 1) / 2 + h;
    return g0 * te[e] + g1 * te[Z::NTES + e] + g2 * te[2 * Z::NTES + e];
  };
  // Be(k, h, j): k = 0: int (Phi_h)_y psi_j ; k = 1: -int (Phi_h)_x psi_j
  const double* vq = a.tables + Z::OFF_VQ + ci * 2 * NH * 3;
  auto Be = [&](int k, int h, int j) {
    const double v0 = vq[h * 3 + j], v1 = vq[(NH + h) * 3 + j];
    return (k == 0) ? (J[1][0] * v0 + J[1][1] * v1) : -(J[0][0] * v0 + J[0][1] * v1);
  };
  // patch-local stress rows from the slots; Lc_e[j] = -int psi_j (s01 - s10), Ce = |detJ|/6
  double* srow[2] = {nullptr, nullptr};
  double Lce[3] = {0.0, 0.0, 0.0};
  if (active)
  {
    const double* sV = a.tables + Z::OFF_V;
    srow[0] = a.out + (((int64_t)0 * a.ncells + cell) * 3 + ln) * NRT;
    srow[1] = a.out + (((int64_t)1 * a.ncells + cell) * 3 + ln) * NRT;
    // grouped patches (modified_patch, se/solve_patch_weaksym.hpp:100-131): own rows + the rows of the
    // group's two-cell patches on this cell
    const uint32_t grows = grouped ? ((info >> INFO_GROUPROW_SHIFT) & 7u) : 0u;
    for (int i = 0; i < NRT; ++i)
    {
      double c0 = srow[0][i], c1 = srow[1][i];
      if (grows)
      {
#pragma unroll
        for (int v = 0; v < 3; ++v)
          if (grows & (1u << v))
          {
            c0 += a.out[(((int64_t)0 * a.ncells + cell) * 3 + v) * NRT + i];
            c1 += a.out[(((int64_t)1 * a.ncells + cell) * 3 + v) * NRT + i];
          }
      }
      const double w0 = c0 * J[1][0] - c1 * J[0][0], w1 = c0 * J[1][1] - c1 * J[0][1];
#pragma unroll
      for (int j = 0; j < 3; ++j)
        Lce[j] -= sgn * (w0 * sV[(j * NRT + i) * 2] + w1 * sV[(j * NRT + i) * 2 + 1]);
    }
  }
  const double Ce = active ? fabs(detJ) / 6.0 : 0.0;

  // ---- numbering: position of the lane's local unknowns [d | um | up | ua] in chain + border order ----
  auto pos_facet = [&](int f, int m) { return (f == 0) ? nch + 1 + m : (f - 1) * (KB + NADD) + NADD + m; };
  int pos[NH];
  pos[0] = nch;
#pragma unroll
  for (int j = 0; j < KB; ++j)
  {
    pos[1 + j] = pos_facet(sub, j);
    pos[1 + KB + j] = pos_facet(fi_p, j);
  }
#pragma unroll
  for (int q = 0; q < NADD; ++q)
    pos[1 + 2 * KB + q] = sub * (KB + NADD) + q;
  // multiplier DOF of the cell's local vertex j (se/Patch.hpp:621-708), as in k_se_weaksym
  const int v_ea = 3 - fp - ln, v_eam1 = 3 - fm - ln;
  int pj[3];
  {
    const int p_ea = interior ? sub + 1 : ((sub + 1 == n) ? nf : sub + 1);
    const int p_eam1 = interior ? ((sub == 0) ? n : sub) : ((sub == 0) ? nf - 1 : sub);
#pragma unroll
    for (int j = 0; j < 3; ++j)
      pj[j] = (j == ln) ? 0 : ((j == v_ea) ? p_ea : ((j == v_eam1) ? p_eam1 : 0));
  }
  // slot of vertex j in a compressed row of B: 0 the patch node, 1 the ring point of the row's facet
  // (of facet s for the bubbles of cell s), 2 / 3 the other ring point of the cell before / after it
  auto bslot = [&](int h, int j) {
    if (j == ln)
      return 0;
    const bool uprow = h > KB && h <= 2 * KB;
    return uprow ? ((j == v_ea) ? 1 : 2) : ((j == v_eam1) ? 1 : 3);
  };
  // fixed (flux-BC) unknowns per row k (se/assembly.hpp:46-98): local unknown h of this lane
  auto fixed = [&](int k, int h) {
    if (!requires_bcs)
      return false;
    if (h == 0)
      return bc0[k] || bcn[k];
    if (h <= KB)
      return bc0[k] && sub == 0;
    if (h <= 2 * KB)
      return bcn[k] && sub == n - 1;
    return false;
  };
  // entry (p, q), p >= q, of the factor buffer
  auto Lref = [&](int p, int q) -> double& {
    return (p < nch) ? band[p * LDB + (p - q)] : bord[(p - nch) * DIMMAX + q];
  };

  // ---- B (both rows), mean-value coupling, right-hand side ----
  for (int e = sub; e < W::FACTOR; e += 64)
    lds[e] = 0.0;
  for (int e = W::OFF_BV + sub; e < W::OFF_Y; e += 64)
    lds[e] = 0.0;
  for (int e = sub; e < W::NINT; e += 64)
    Bp[e] = 0;
  wave_sync();
  if (active)
  {
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int h = 0; h < NH; ++h)
      {
        if (fixed(k, h))
          continue; // rows of fixed unknowns are dropped (se/assembly.hpp:430-436)
#pragma unroll
        for (int j = 0; j < 3; ++j)
        {
          const double v = Be(k, h, j);
          if (h == 0)
            atomicAdd(&Bd[k * NPMAX + pj[j]], v);
          else
            atomicAdd(&Bv[(k * DIMMAX + pos[h]) * 4 + bslot(h, j)], v);
        }
      }
#pragma unroll
    for (int h = 1; h < NH; ++h)
#pragma unroll
      for (int j = 0; j < 3; ++j)
      {
        const int s = bslot(h, j);
        if (s > 0)
          atomicOr(&Bp[pos[h]], pj[j] << (8 * (s - 1)));
      }
#pragma unroll
    for (int j = 0; j < 3; ++j)
    {
      atomicAdd(&Rg[pj[j]], Lce[j]);
      if (meanvalue)
      {
        atomicAdd(&Cg[pj[j] * DCMAX + npnt], Ce);
        atomicAdd(&Cg[npnt * DCMAX + pj[j]], Ce);
      }
    }
  }
  wave_sync();

  int status_local = 0;
  // ---- A_k (masked for row k) into the factor buffer and its Cholesky factor ----
  auto factor = [&](int k) {
    for (int e = sub; e < W::FACTOR; e += 64)
      lds[e] = 0.0;
    wave_sync();
    if (active)
    {
#pragma unroll
      for (int h = 0; h < NH; ++h)
      {
        if (fixed(k, h))
          continue;
#pragma unroll
        for (int g = 0; g < NH; ++g)
          if (pos[h] >= pos[g] && !fixed(k, g))
            atomicAdd(&Lref(pos[h], pos[g]), Te(h, g));
      }
    }
    wave_sync();
    if (requires_bcs && sub == 0) // identity rows of the fixed unknowns
    {
      if (bc0[k] || bcn[k])
        bord[nch] = 1.0;
      for (int m = 0; m < KB; ++m)
      {
        if (bc0[k])
          Lref(nch + 1 + m, nch + 1 + m) = 1.0;
        if (bcn[k])
          Lref(pos_facet(n, m), pos_facet(n, m)) = 1.0;
      }
    }
    wave_sync();
    // chain columns: right-looking, the update of column j touches the BW band rows below it and the
    // border rows; pair e of the (BW + NBD)(BW + NBD + 1)/2 updated entries is fixed per lane
    constexpr int NT = BW + NBD, NPAIR = NT * (NT + 1) / 2, NPL = (NPAIR + 63) / 64;
    int pa[NPL], pb[NPL];
#pragma unroll
    for (int t = 0; t < NPL; ++t)
    {
      const int e = sub + 64 * t;
      int r = 0;
      while ((r + 1) * (r + 2) / 2 <= e)
        ++r;
      pa[t] = (e < NPAIR) ? r : -1;
      pb[t] = e - r * (r + 1) / 2;
    }
    for (int j = 0; j < nch; ++j)
    {
      const double ajj = band[j * LDB];
      if (!(ajj > 0.0) || !isfinite(ajj))
        status_local = 1;
      const double inv = rsqrt_d((ajj > 0.0) ? ajj : 1.0);
      wave_sync();
      if (sub == 0)
      {
        band[j * LDB] = ((ajj > 0.0) ? ajj : 1.0) * inv;
        dinv[j] = inv;
      }
      else if (sub <= BW)
      {
        if (j + sub < nch)
          band[(j + sub) * LDB + sub] *= inv;
      }
      else if (sub <= BW + NBD)
        bord[(sub - BW - 1) * DIMMAX + j] *= inv;
      wave_sync();
#pragma unroll
      for (int t = 0; t < NPL; ++t)
      {
        if (pa[t] < 0)
          continue;
        // member r of the updated set: chain row j + 1 + r (r < BW) or border row r - BW
        const int ra = pa[t], rb = pb[t];
        const int p = (ra < BW) ? j + 1 + ra : nch + ra - BW, q = (rb < BW) ? j + 1 + rb : nch + rb - BW;
        if (p < nch + NBD && (ra >= BW || p < nch) && (rb >= BW || q < nch))
          Lref(p, q) -= Lref(p, j) * Lref(q, j);
      }
      wave_sync();
    }
    // dense border block
    if (sub == 0)
    {
      for (int j = 0; j < NBD; ++j)
      {
        double* lj = bord + j * DIMMAX + nch;
        const double ajj = lj[j];
        if (!(ajj > 0.0) || !isfinite(ajj))
          status_local = 1;
        const double inv = rsqrt_d((ajj > 0.0) ? ajj : 1.0);
        lj[j] = ((ajj > 0.0) ? ajj : 1.0) * inv;
        dinv[nch + j] = inv;
        for (int i = j + 1; i < NBD; ++i)
          bord[i * DIMMAX + nch + j] *= inv;
        for (int i = j + 1; i < NBD; ++i)
          for (int kk = j + 1; kk <= i; ++kk)
            bord[i * DIMMAX + nch + kk] -= bord[i * DIMMAX + nch + j] * bord[kk * DIMMAX + nch + j];
      }
    }
    wave_sync();
  };

  // row of B_k at position q, column (point) c
  auto Bat = [&](int k, int q, int c) {
    if (q == nch)
      return Bd[k * NPMAX + c];
    const double* bv = Bv + (k * DIMMAX + q) * 4;
    const int pk = Bp[q];
    double b = (c == 0) ? bv[0] : 0.0;
    b += ((pk & 255) == c) ? bv[1] : 0.0;
    b += (((pk >> 8) & 255) == c) ? bv[2] : 0.0;
    b += (((pk >> 16) & 255) == c) ? bv[3] : 0.0;
    return b;
  };
  // S -= sum over nr buffered rows of Y_k^T Y_k (k = kf, or both rows for kf < 0)
  auto fold = [&](int nr, int kf) {
    wave_sync();
    for (int e = sub; e < npnt * npnt; e += 64)
    {
      const int r = e / npnt, c = e - r * npnt;
      double t = 0.0;
      for (int i = 0; i < nr; ++i)
#pragma unroll
        for (int k = 0; k < 2; ++k)
          if (kf < 0 || kf == k)
            t += Yb[i * LDY + k * NPMAX + r] * Yb[i * LDY + k * NPMAX + c];
      Cg[r * DCMAX + c] -= t;
    }
    wave_sync();
  };
  // ---- Y_k = L_k^-1 B_k, folded into S: lane columns col = sub + 64 t of [B_0 | B_1] (or of B_kf) ----
  auto schur = [&](int kf) {
    const int ncols = (kf < 0) ? 2 * npnt : npnt;
    int ck[NCT], cc[NCT];
    bool cv[NCT];
    double win[NCT][BW], acc[NCT][NBD];
#pragma unroll
    for (int t = 0; t < NCT; ++t)
    {
      const int col = sub + 64 * t;
      cv[t] = col < ncols;
      ck[t] = cv[t] ? ((kf < 0) ? col / npnt : kf) : 0;
      cc[t] = cv[t] ? ((kf < 0) ? col - ck[t] * npnt : col) : 0;
#pragma unroll
      for (int d = 0; d < BW; ++d)
        win[t][d] = 0.0;
#pragma unroll
      for (int b = 0; b < NBD; ++b)
        acc[t][b] = 0.0;
    }
    for (int i0 = 0; i0 < nch; i0 += RCH)
    {
      const int nr = (nch - i0 < RCH) ? nch - i0 : RCH;
      for (int r = 0; r < nr; ++r)
      {
        const int i = i0 + r;
        double l[BW], lb[NBD];
#pragma unroll
        for (int d = 0; d < BW; ++d)
          l[d] = (d + 1 <= i) ? band[i * LDB + d + 1] : 0.0;
#pragma unroll
        for (int b = 0; b < NBD; ++b)
          lb[b] = bord[b * DIMMAX + i];
        const double di = dinv[i];
#pragma unroll
        for (int t = 0; t < NCT; ++t)
        {
          double y = cv[t] ? Bat(ck[t], i, cc[t]) : 0.0;
#pragma unroll
          for (int d = 0; d < BW; ++d)
            y -= l[d] * win[t][d];
          y *= di;
#pragma unroll
          for (int d = BW - 1; d > 0; --d)
            win[t][d] = win[t][d - 1];
          win[t][0] = y;
#pragma unroll
          for (int b = 0; b < NBD; ++b)
            acc[t][b] += lb[b] * y;
          if (cv[t])
            Yb[r * LDY + ck[t] * NPMAX + cc[t]] = y;
        }
      }
      fold(nr, kf);
    }
    // border rows
    double yb[NCT][NBD];
    for (int b = 0; b < NBD; ++b)
    {
      double lbb[NBD];
#pragma unroll
      for (int q = 0; q < NBD; ++q)
        lbb[q] = (q < b) ? bord[b * DIMMAX + nch + q] : 0.0;
      const double di = dinv[nch + b];
#pragma unroll
      for (int t = 0; t < NCT; ++t)
      {
        double y = (cv[t] ? Bat(ck[t], nch + b, cc[t]) : 0.0) - acc[t][b];
#pragma unroll
        for (int q = 0; q < NBD; ++q)
          if (q < b)
            y -= lbb[q] * yb[t][q];
        y *= di;
        yb[t][b] = y;
        if (cv[t])
          Yb[b * LDY + ck[t] * NPMAX + cc[t]] = y;
      }
    }
    fold(NBD, kf);
  };

  // ---- u_k = -A_k^-1 (B_k gamma) into w_k = Yb + k DIMMAX (lane sub == k, or the lane of kf) ----
  auto solve_u = [&](int kf) {
    double* wv = Yb;
    for (int e = sub; e < 2 * dim; e += 64)
    {
      const int k = e / dim, q = e - k * dim;
      if (kf >= 0 && k != kf)
        continue;
      double t = 0.0;
      if (q == nch)
      {
        for (int c = 0; c < npnt; ++c)
          t += Bd[k * NPMAX + c] * Gg[c];
      }
      else
      {
        const double* bv = Bv + (k * DIMMAX + q) * 4;
        const int pk = Bp[q];
        t = bv[0] * Gg[0] + bv[1] * Gg[pk & 255] + bv[2] * Gg[(pk >> 8) & 255] + bv[3] * Gg[(pk >> 16) & 255];
      }
      wv[k * DIMMAX + q] = -t;
    }
    wave_sync();
    if ((kf < 0 && sub < 2) || sub == kf)
    {
      double* w = wv + sub * DIMMAX;
      for (int i = 0; i < nch; ++i)
      {
        double t = w[i];
        for (int d = 1; d <= BW && d <= i; ++d)
          t -= band[i * LDB + d] * w[i - d];
        w[i] = t * dinv[i];
      }
      for (int b = 0; b < NBD; ++b)
      {
        double t = w[nch + b];
        for (int q = 0; q < nch + b; ++q)
          t -= bord[b * DIMMAX + q] * w[q];
        w[nch + b] = t * dinv[nch + b];
      }
      for (int b = NBD - 1; b >= 0; --b)
      {
        double t = w[nch + b];
        for (int q = b + 1; q < NBD; ++q)
          t -= bord[q * DIMMAX + nch + b] * w[nch + q];
        w[nch + b] = t * dinv[nch + b];
      }
      for (int i = nch - 1; i >= 0; --i)
      {
        double t = w[i];
        for (int d = 1; d <= BW && i + d < nch; ++d)
          t -= band[(i + d) * LDB + d] * w[i + d];
        for (int b = 0; b < NBD; ++b)
          t -= bord[b * DIMMAX + i] * w[nch + b];
        w[i] = t * dinv[i];
      }
    }
    wave_sync();
  };

  // ---- Schur complement S (C = M - S) ----
  if (!requires_bcs)
  {
    factor(0);
    schur(-1);
  }
  else
  {
    factor(0);
    schur(0);
    factor(1);
    schur(1);
  }

  // ---- Gauss-Jordan with row pivoting of the (npnt [+1])^2 Schur system, with the rank-revealing
  // threshold of k_se_weaksym: the multiplier of a column without pivot is 0 ----
  {
    double cscale = 0.0;
    for (int e = sub; e < dim_c * dim_c; e += 64)
    {
      const double v = Cg[(e / dim_c) * DCMAX + e % dim_c];
      if (!isfinite(v))
        status_local = 1;
      cscale = fmax(cscale, fabs(v));
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1)
      cscale = fmax(cscale, __shfl_xor(cscale, off, 64));
    const double ptol = EQLB_WS_PIVOT_RTOL * cscale;
    int nr = 0; // rows used so far
    for (int c = 0; c < dim_c; ++c)
    {
      // first row of largest modulus among the rows not used yet
      double bv = -1.0;
      int br = DCMAX;
      for (int r = nr + sub; r < dim_c; r += 64)
      {
        const double v = fabs(Cg[r * DCMAX + c]);
        if (v > bv)
        {
          bv = v;
          br = r;
        }
      }
#pragma unroll
      for (int off = 1; off < 64; off <<= 1)
      {
        const double ov = __shfl_xor(bv, off, 64);
        const int orow = __shfl_xor(br, off, 64);
        if (ov > bv || (ov == bv && orow < br))
        {
          bv = ov;
          br = orow;
        }
      }
      if (!(bv > ptol))
      {
        if (sub == 0)
          pcol[c] = -1;
        continue;
      }
      if (!isfinite(bv))
        status_local = 1;
      if (br != nr)
      {
        for (int j = sub; j <= dim_c; j += 64)
        {
          double* x = (j < dim_c) ? Cg + nr * DCMAX + j : Rg + nr;
          double* y = (j < dim_c) ? Cg + br * DCMAX + j : Rg + br;
          const double t = *x;
          *x = *y;
          *y = t;
        }
        wave_sync();
      }
      const double ip = 1.0 / Cg[nr * DCMAX + c];
      for (int r = nr + 1 + sub; r < dim_c; r += 64)
      {
        const double f = Cg[r * DCMAX + c] * ip;
        for (int j = c; j < dim_c; ++j)
          Cg[r * DCMAX + j] -= f * Cg[nr * DCMAX + j];
        Rg[r] -= f * Rg[nr];
      }
      if (sub == 0)
        pcol[c] = nr;
      ++nr;
      wave_sync();
    }
    // back substitution over the pivot columns, right to left
    if (sub == 0)
    {
      for (int c = dim_c - 1; c >= 0; --c)
      {
        if (pcol[c] < 0)
        {
          Gg[c] = 0.0;
          continue;
        }
        const int r = pcol[c];
        double t = Rg[r];
        for (int j = c + 1; j < dim_c; ++j)
          t -= Cg[r * DCMAX + j] * Gg[j];
        Gg[c] = t / Cg[r * DCMAX + c];
        if (!isfinite(Gg[c]))
          status_local = 1;
      }
    }
    wave_sync();
  }

  if (!requires_bcs)
    solve_u(-1);
  else
  {
    solve_u(1); // A_1 is the factor in the buffer
    factor(0);
    solve_u(0);
  }

  // ---- back-map and add to the slot rows (se/solve_patch_weaksym.hpp:189-232) ----
  if (active)
  {
#pragma unroll
    for (int k = 0; k < 2; ++k)
    {
      const double* w = Yb + k * DIMMAX;
      double ul[NH];
#pragma unroll
      for (int h = 0; h < NH; ++h)
        ul[h] = w[pos[h]];
      double* o = srow[k];
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
  }
  if (status_local)
    atomicOr(a.status, 2);
}

template <int K, int P>
static int launch_ws_banded_t(const SeArgs& a, hipStream_t stream)
{
  using W = WsBand<K, P>;
  const size_t lds_bytes = sizeof(double) * (size_t)W::lds_doubles();
  static_assert(sizeof(double) * W::lds_doubles() <= 160 * 1024, "banded weak-symmetry kernel: LDS");
  auto kern = k_se_weaksym_banded<K, P>;
  if (lds_bytes > 64 * 1024)
  {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes)
        != hipSuccess)
      return EQLB_ERR_DEVICE;
  }
  if (a.npatch == 0)
    return 0;
  hipLaunchKernelGGL(kern, dim3((unsigned)a.npatch), dim3(64), lds_bytes, stream, a);
  return (hipGetLastError() == hipSuccess) ? 0 : EQLB_ERR_DEVICE;
}

int launch_se_weaksym_banded(int k, int P, const SeArgs& a, hipStream_t stream)
{
  if (k == 4 && P == 16)
    return launch_ws_banded_t<4, 16>(a, stream);
  if (k == 4 && P == 32)
    return launch_ws_banded_t<4, 32>(a, stream);
  if (k == 4 && P == 64)
    return launch_ws_banded_t<4, 64>(a, stream);
  if (k == 3 && P == 64)
    return launch_ws_banded_t<3, 64>(a, stream);
  return EQLB_ERR_UNSUPPORTED;
}

} // namespace eqlb
