// Weak symmetry of equilibrated stresses for the large bins: RT_4 with patches of 9 ... 64 facets and RT_3
// with 33 ... 64 facets.  The contract is that of eqlb_se_weaksym_common.h; against k_se_weaksym the LDS grows
// linearly with the patch instead of quadratically, so these bins fit a workgroup.
//
// One patch per wave (64 lanes; lane i <-> cell T_{i+1}).  The unknowns of the patch are ordered as a
// banded chain plus a border (WsChain, eqlb_se_weaksym_numbering.h: chain [a_0 | x_1 | a_1 | ...], border [d | x_0]).
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
#include "eqlb_se_weaksym_common.h"
#include "eqlb_tables_gen.h"

namespace eqlb
{

template <int K, int P>
struct WsBand : WsChain<K>
{
  using Z = Sizes<K, K - 1, P>;
  using C = WsChain<K>;
  static constexpr int KB = C::KB, NADD = C::NADD, NH = C::NH, NBD = C::NBD, BW = C::BW, LDB = C::LDB;
  static constexpr int DIMMAX = Z::DIMMAX;     // H(div=0) unknowns of a patch
  static constexpr int NCHMAX = DIMMAX - NBD;  // chain
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
  constexpr int KB = W::KB, NH = W::NH, NBD = W::NBD, BW = W::BW, LDB = W::LDB;
  constexpr int DIMMAX = W::DIMMAX, NPMAX = W::NPMAX, DCMAX = W::DCMAX, LDY = W::LDY, RCH = W::RCH;
  constexpr int NCT = W::NCT;

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
  const WsPatch pt = ws_patch(flag0, a.pflag[a.npatch_total + patch], (int)a.pn[patch]);
  const int n = pt.n, npnt = pt.npnt, dim_c = pt.dim_c;
  const bool requires_bcs = pt.requires_bcs, meanvalue = pt.meanvalue;
  const int dim = W::dim(pt), nch = W::nch(pt);
  const bool active = sub < n;
  // the lane's cell; the tables are read from global memory: they would cost the LDS of a patch
  const WsCell<K> cell(a, a.tables + Z::OFF_TE, a.tables + Z::OFF_VQ, slot, active, pt, sub);
  // patch-local stress rows from the slots; Lc_e[j] = -int psi_j (s01 - s10), Ce = |detJ|/6
  double Lce[3] = {0.0, 0.0, 0.0};
  if (active)
    cell.template load<false>(a.out, a.ncells, grouped, a.tables + Z::OFF_V, Lce);
  const double Ce = active ? cell.Ce() : 0.0;

  // ---- numbering: position of the lane's local unknowns [d | um | up | ua] in chain + border order ----
  auto pos_facet = [&](int f, int m) { return W::pos_facet(nch, f, m); };
  int pos[NH];
  W::pos(pt, sub, pos);
  const int pj[3] = {cell.pj(0), cell.pj(1), cell.pj(2)};
  auto bslot = [&](int h, int j) { return W::bslot(cell.fm, cell.fp, cell.ln, h, j); };
  auto fixed = [&](int k, int h) { return W::fixed(pt, k, h, sub); };
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
          const double v = cell.Be(k, h, j);
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
            atomicAdd(&Lref(pos[h], pos[g]), cell.Te(h, g));
      }
    }
    wave_sync();
    if (requires_bcs && sub == 0) // identity rows of the fixed unknowns
    {
      if (pt.bc0(k) || pt.bcn(k))
        bord[nch] = 1.0;
      for (int m = 0; m < KB; ++m)
      {
        if (pt.bc0(k))
          Lref(nch + 1 + m, nch + 1 + m) = 1.0;
        if (pt.bcn(k))
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
    if (sub == 0)
      ws_back_substitute(Cg, DCMAX, Rg, pcol, dim_c, Gg, &status_local);
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

  // ---- back-map and add to the slot rows ----
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
      cell.add_correction(ul, cell.row(a.out, a.ncells, k));
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
  if (!ws_allow_lds(kern, lds_bytes))
    return EQLB_ERR_DEVICE;
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
