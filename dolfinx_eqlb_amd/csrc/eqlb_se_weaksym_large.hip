// Weak symmetry of equilibrated stresses on vertex patches that do not fit one wavefront (more than 63 cells or more
// than 64 patch facets; option "large_patches_stress"): one WORKGROUP per patch, the cells of the fan strided over its
// threads.  The contract is that of eqlb_se_weaksym_common.h, the formulation that of k_se_weaksym_banded
// (eqlb_se_weaksym_banded.hip) - the patch unknowns as a banded chain plus a border (WsChain), the Cholesky factor in
// that profile, B_k in compressed rows, S = sum_k Y_k^T Y_k folded chunk by chunk without storing Y - carried to a
// workgroup the way k_se_patch_large (eqlb_se_large.hip) carries the flux:
//   * nothing assumes lane = cell; the cell count is the difference of the CSR offsets of the large-patch SoA
//   * everything whose size grows with the patch - band, border rows, compressed B, Schur matrix, right-hand sides, the
//     sliding windows of the forward substitution - lives in a global work space sized at eqlb_se_set_boundary
//     (large_patch_weaksym_ws_doubles); threads hand data over through it across __syncthreads().  LDS: the few words
//     of the block reductions, independent of the patch
//   * no floating-point atomics: cells that share a matrix entry (neighbours in the fan share a facet) assemble in
//     different phases (even cells, odd cells, the last cell of a fan with an odd count), what every cell adds to
//     (the patch node) is summed over the cells by one thread.  All sums run in a fixed order: two calls give the same
//     bits
// The kernel reads the patch-local rows of right-hand sides 0 and 1 that k_se_patch_large wrote into the slot buffer
// and adds the corrections in place.  A large patch is never part of a group of boundary patches (refused at
// eqlb_se_set_boundary), so there is one pass and no row of another patch is read.
// It is a coverage path: the columns of the factorisation and of the elimination are barriers apart.
#include "eqlb_se_weaksym_common.h"

namespace eqlb
{

namespace
{
constexpr int WL_BLOCK = 256;

// work space of one patch of n cells (doubles), laid out for the larger of the two cases (boundary patch: n + 1 facets)
template <int K>
struct WsLarge : WsChain<K>
{
  using Z = Sizes<K, K - 1, 64>;
  using C = WsChain<K>;
  static constexpr int KB = C::KB, NADD = C::NADD, NH = C::NH, NBD = C::NBD, BW = C::BW, LDB = C::LDB;
  static constexpr int RCH = 16;               // rows of Y per chunk
  static constexpr int NWIN = BW + NBD;        // per column of B: window of the chain + sums of the border rows
  static constexpr int NCB = 5;                // per cell: Te(d, d) | B_0(d, node) | B_1(d, node) | load(node) | |T|/6
  static_assert(NBD <= RCH, "the border rows go through the Y buffer");
  int64_t dimm, npm, dcm; // H(div=0) unknowns, patch points, multipliers (+ mean value): upper bounds
  int64_t band, bord, dinv, factor_end, bv, bp, bd, c, r, g, pcol, fac, win, y, cb, hd, total;
  __host__ __device__ explicit WsLarge(int64_t n)
  {
    dimm = 1 + (int64_t)KB * (n + 1) + (int64_t)NADD * n;
    npm = n + 2;
    dcm = npm + 1;
    band = 0;
    bord = band + dimm * LDB;
    dinv = bord + NBD * dimm;
    factor_end = dinv + dimm;
    bv = factor_end;           // [2][dimm][4]
    bp = bv + 2 * dimm * 4;    // int [dimm][4]: ring points of the B slots 1 ... 3
    bd = bp + 2 * dimm;        // [2][npm]
    c = bd + 2 * npm;          // [dcm][dcm]
    r = c + dcm * dcm;
    g = r + dcm;
    pcol = g + dcm;            // int [dcm]
    fac = pcol + dcm;
    win = fac + dcm;           // [2 npm][NWIN]
    y = win + 2 * npm * NWIN;  // [RCH][2 npm], later w [2][dimm]
    const int64_t ny = (RCH * 2 * npm > 2 * dimm) ? RCH * 2 * npm : 2 * dimm;
    cb = y + ny;               // [n][NCB]
    hd = cb + n * NCB;         // header: sum of Te(d, d)
    total = hd + 2;
  }
};

struct WsLargeArgs
{
  const int32_t* off;   // [npatch + 1] first lane slot of the patch (CSR)
  const int64_t* wsoff; // [npatch] first double of the patch's work space
  double* ws;
};

// maximum over the workgroup, result in every thread (red: WL_BLOCK / 64 doubles of LDS)
__device__ __forceinline__ double block_max(double v, double* red, int tid)
{
#pragma unroll
  for (int off = 1; off < 64; off <<= 1)
    v = fmax(v, __shfl_xor(v, off, 64));
  __syncthreads();
  if ((tid & 63) == 0)
    red[tid >> 6] = v;
  __syncthreads();
  double m = red[0];
#pragma unroll
  for (int w = 1; w < WL_BLOCK / 64; ++w)
    m = fmax(m, red[w]);
  return m;
}

template <int K>
__global__ void __launch_bounds__(WL_BLOCK) k_se_weaksym_large(const SeArgs a, const WsLargeArgs la)
{
  using W = WsLarge<K>;
  using Z = typename W::Z;
  constexpr int KB = W::KB, NH = W::NH, NBD = W::NBD, BW = W::BW, LDB = W::LDB;
  constexpr int RCH = W::RCH, NWIN = W::NWIN, NCB = W::NCB;
  __shared__ double red_v[WL_BLOCK / 64];
  __shared__ int red_i[WL_BLOCK / 64];

  const int patch = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t s0 = la.off[patch];
  const int n = (int)(la.off[patch + 1] - s0);
  const WsPatch pt = ws_patch(a.pflag[patch], a.pflag[a.npatch_total + patch], n);
  const int npnt = pt.npnt, dim_c = pt.dim_c;
  const bool requires_bcs = pt.requires_bcs, meanvalue = pt.meanvalue;
  const int dim = W::dim(pt), nch = W::nch(pt);

  const W L(n);
  const int64_t dimm = L.dimm, npm = L.npm, dcm = L.dcm, LDY = 2 * L.npm;
  double* const wsp = la.ws + la.wsoff[patch];
  double* const band = wsp + L.band;
  double* const bord = wsp + L.bord;
  double* const dinv = wsp + L.dinv;
  double* const Bv = wsp + L.bv;
  int* const Bp = reinterpret_cast<int*>(wsp + L.bp);
  double* const Bd = wsp + L.bd;
  double* const Cg = wsp + L.c;
  double* const Rg = wsp + L.r;
  double* const Gg = wsp + L.g;
  int* const pcol = reinterpret_cast<int*>(wsp + L.pcol);
  double* const fac = wsp + L.fac;
  double* const win = wsp + L.win;
  double* const Yb = wsp + L.y;
  double* const cb = wsp + L.cb;
  double* const hd = wsp + L.hd;

  // ---- what a thread knows of cell i of the fan is recomputed where it is needed: nothing is kept per lane ----
  const double* const te_table = a.tables + Z::OFF_TE;
  const double* const vq_table = a.tables + Z::OFF_VQ;
  auto pos_facet = [&](int f, int m) { return W::pos_facet(nch, f, m); };
  // Neighbours in the fan share the unknowns of a facet, the first and the last cell of a ring those of facet 0:
  // the cells of one phase share no entry but those of the patch node
  auto phase_of = [&](int i) { return ((n & 1) && i == n - 1) ? 2 : (i & 1); };
  // entry (p, q), p >= q, of the factor buffer
  auto Lref = [&](int p, int q) -> double& {
    return (p < nch) ? band[(int64_t)p * LDB + (p - q)] : bord[(int64_t)(p - nch) * dimm + q];
  };

  // ---- B (both rows), mean-value coupling, right-hand side ----
  for (int64_t e = L.factor_end + tid; e < L.total; e += WL_BLOCK)
    wsp[e] = 0.0;
  __syncthreads();
  for (int ph = 0; ph < 3; ++ph)
  {
    for (int i = tid; i < n; i += WL_BLOCK)
    {
      if (phase_of(i) != ph)
        continue;
      const WsCell<K> c(a, te_table, vq_table, s0 + i, true, pt, i);
      int pos[NH];
      W::pos(pt, i, pos);
      // patch-local stress rows from the slots; Lc_e[j] = -int psi_j (s01 - s10), Ce = |detJ|/6
      double Lce[3] = {0.0, 0.0, 0.0};
      c.template load<false>(a.out, a.ncells, false, a.tables + Z::OFF_V, Lce);
      const double Ce = c.Ce();
      double cbv[NCB] = {c.Te(0, 0), 0.0, 0.0, 0.0, Ce};
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int h = 0; h < NH; ++h)
        {
          if (W::fixed(pt, k, h, i))
            continue; // rows of fixed unknowns are dropped (se/assembly.hpp:430-436)
#pragma unroll
          for (int j = 0; j < 3; ++j)
          {
            const double v = c.Be(k, h, j);
            if (h == 0)
            {
              if (j == c.ln)
                cbv[1 + k] = v;
              else
                Bd[k * npm + c.pj(j)] += v;
            }
            else
              Bv[((int64_t)k * dimm + pos[h]) * 4 + W::bslot(c.fm, c.fp, c.ln, h, j)] += v;
          }
        }
#pragma unroll
      for (int h = 1; h < NH; ++h)
#pragma unroll
        for (int j = 0; j < 3; ++j)
        {
          const int s = W::bslot(c.fm, c.fp, c.ln, h, j);
          if (s > 0)
            Bp[(int64_t)pos[h] * 4 + (s - 1)] = c.pj(j);
        }
#pragma unroll
      for (int j = 0; j < 3; ++j)
      {
        if (j == c.ln)
        {
          cbv[3] = Lce[j];
          continue;
        }
        Rg[c.pj(j)] += Lce[j];
        if (meanvalue)
        {
          Cg[c.pj(j) * dcm + npnt] += Ce;
          Cg[npnt * dcm + c.pj(j)] += Ce;
        }
      }
#pragma unroll
      for (int q = 0; q < NCB; ++q)
        cb[(int64_t)i * NCB + q] = cbv[q];
    }
    __syncthreads();
  }
  if (tid == 0)
  {
    // what every cell adds to: the entries of the patch node, in fan order
    double s[NCB] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < n; ++i)
#pragma unroll
      for (int q = 0; q < NCB; ++q)
        s[q] += cb[(int64_t)i * NCB + q];
    hd[0] = s[0];
    Bd[0] = s[1];
    Bd[npm] = s[2];
    Rg[0] = s[3];
    if (meanvalue)
    {
      Cg[npnt] = s[4];
      Cg[npnt * dcm] = s[4];
    }
  }
  __syncthreads();

  int status_local = 0;
  // ---- A_k (masked for row k) into the factor buffer and its Cholesky factor ----
  auto factor = [&](int k) {
    for (int64_t e = tid; e < L.factor_end; e += WL_BLOCK)
      wsp[e] = 0.0;
    __syncthreads();
    for (int ph = 0; ph < 3; ++ph)
    {
      for (int i = tid; i < n; i += WL_BLOCK)
      {
        if (phase_of(i) != ph)
          continue;
        const WsCell<K> c(a, te_table, vq_table, s0 + i, true, pt, i);
        int pos[NH];
        W::pos(pt, i, pos);
#pragma unroll
        for (int h = 0; h < NH; ++h)
        {
          if (W::fixed(pt, k, h, i))
            continue;
#pragma unroll
          for (int g = 0; g < NH; ++g)
            if (pos[h] >= pos[g] && !W::fixed(pt, k, g, i) && (h > 0 || g > 0))
              Lref(pos[h], pos[g]) += c.Te(h, g);
        }
      }
      __syncthreads();
    }
    if (tid == 0)
    {
      // the patch node: sum over the cells, or the identity row of a fixed unknown; identity rows of the fixed facets
      const bool dfix = requires_bcs && (pt.bc0(k) || pt.bcn(k));
      bord[nch] = dfix ? 1.0 : hd[0];
      if (requires_bcs)
        for (int m = 0; m < KB; ++m)
        {
          if (pt.bc0(k))
            Lref(nch + 1 + m, nch + 1 + m) = 1.0;
          if (pt.bcn(k))
            Lref(pos_facet(n, m), pos_facet(n, m)) = 1.0;
        }
    }
    __syncthreads();
    // chain columns: right-looking, the update of column j touches the BW band rows below it and the border rows;
    // thread e takes pair e of the (BW + NBD)(BW + NBD + 1)/2 updated entries.  (The diagonal of the factor is kept
    // as its reciprocal in dinv only: nothing reads it from the band.)
    constexpr int NT = BW + NBD, NPAIR = NT * (NT + 1) / 2;
    static_assert(NPAIR <= WL_BLOCK, "one updated entry per thread");
    int ra = 0;
    while ((ra + 1) * (ra + 2) / 2 <= tid)
      ++ra;
    const int rb = tid - ra * (ra + 1) / 2;
    for (int j = 0; j < nch; ++j)
    {
      const double ajj = band[(int64_t)j * LDB];
      if (!(ajj > 0.0) || !isfinite(ajj))
        status_local = 1;
      const double inv = rsqrt_d((ajj > 0.0) ? ajj : 1.0);
      if (tid == 0)
        dinv[j] = inv;
      else if (tid <= BW)
      {
        if (j + tid < nch)
          band[(int64_t)(j + tid) * LDB + tid] *= inv;
      }
      else if (tid <= BW + NBD)
        bord[(int64_t)(tid - BW - 1) * dimm + j] *= inv;
      __syncthreads();
      if (tid < NPAIR)
      {
        // member r of the updated set: chain row j + 1 + r (r < BW) or border row r - BW
        const int p = (ra < BW) ? j + 1 + ra : nch + ra - BW, q = (rb < BW) ? j + 1 + rb : nch + rb - BW;
        if ((ra >= BW || p < nch) && (rb >= BW || q < nch))
          Lref(p, q) -= Lref(p, j) * Lref(q, j);
      }
      __syncthreads();
    }
    // dense border block
    if (tid == 0)
    {
      for (int j = 0; j < NBD; ++j)
      {
        double* lj = bord + (int64_t)j * dimm + nch;
        const double ajj = lj[j];
        if (!(ajj > 0.0) || !isfinite(ajj))
          status_local = 1;
        const double inv = rsqrt_d((ajj > 0.0) ? ajj : 1.0);
        lj[j] = ((ajj > 0.0) ? ajj : 1.0) * inv;
        dinv[nch + j] = inv;
        for (int i = j + 1; i < NBD; ++i)
          bord[(int64_t)i * dimm + nch + j] *= inv;
        for (int i = j + 1; i < NBD; ++i)
          for (int kk = j + 1; kk <= i; ++kk)
            bord[(int64_t)i * dimm + nch + kk] -= bord[(int64_t)i * dimm + nch + j] * bord[(int64_t)kk * dimm + nch + j];
      }
    }
    __syncthreads();
  };

  // row of B_k at position q, column (point) c
  auto Bat = [&](int k, int q, int c) {
    if (q == nch)
      return Bd[k * npm + c];
    const double* bv = Bv + ((int64_t)k * dimm + q) * 4;
    const int* pk = Bp + (int64_t)q * 4;
    double b = (c == 0) ? bv[0] : 0.0;
    b += (pk[0] == c) ? bv[1] : 0.0;
    b += (pk[1] == c) ? bv[2] : 0.0;
    b += (pk[2] == c) ? bv[3] : 0.0;
    return b;
  };
  // S -= sum over nr buffered rows of Y_k^T Y_k (k = kf, or both rows for kf < 0)
  auto fold = [&](int nr, int kf) {
    __syncthreads();
    for (int64_t e = tid; e < (int64_t)npnt * npnt; e += WL_BLOCK)
    {
      const int64_t r = e / npnt, c = e - r * npnt;
      double t = 0.0;
      for (int i = 0; i < nr; ++i)
#pragma unroll
        for (int k = 0; k < 2; ++k)
          if (kf < 0 || kf == k)
            t += Yb[i * LDY + k * npm + r] * Yb[i * LDY + k * npm + c];
      Cg[r * dcm + c] -= t;
    }
    __syncthreads();
  };
  // ---- Y_k = L_k^-1 B_k, folded into S: the columns of [B_0 | B_1] (or of B_kf) strided over the threads; a column
  // keeps the last BW values of its forward substitution and its sums over the border rows in the work space ----
  auto schur = [&](int kf) {
    const int ncols = (kf < 0) ? 2 * npnt : npnt;
    for (int64_t e = tid; e < (int64_t)ncols * NWIN; e += WL_BLOCK)
      win[e] = 0.0;
    __syncthreads();
    for (int i0 = 0; i0 < nch; i0 += RCH)
    {
      const int nr = (nch - i0 < RCH) ? nch - i0 : RCH;
      for (int col = tid; col < ncols; col += WL_BLOCK)
      {
        const int ck = (kf < 0) ? col / npnt : kf;
        const int cc = (kf < 0) ? col - ck * npnt : col;
        double* wc = win + (int64_t)col * NWIN;
        double wv[BW], acc[NBD];
#pragma unroll
        for (int d = 0; d < BW; ++d)
          wv[d] = wc[d];
#pragma unroll
        for (int b = 0; b < NBD; ++b)
          acc[b] = wc[BW + b];
        for (int r = 0; r < nr; ++r)
        {
          const int i = i0 + r;
          double y = Bat(ck, i, cc);
#pragma unroll
          for (int d = 0; d < BW; ++d)
            y -= ((d + 1 <= i) ? band[(int64_t)i * LDB + d + 1] : 0.0) * wv[d];
          y *= dinv[i];
#pragma unroll
          for (int d = BW - 1; d > 0; --d)
            wv[d] = wv[d - 1];
          wv[0] = y;
#pragma unroll
          for (int b = 0; b < NBD; ++b)
            acc[b] += bord[(int64_t)b * dimm + i] * y;
          Yb[r * LDY + ck * npm + cc] = y;
        }
#pragma unroll
        for (int d = 0; d < BW; ++d)
          wc[d] = wv[d];
#pragma unroll
        for (int b = 0; b < NBD; ++b)
          wc[BW + b] = acc[b];
      }
      fold(nr, kf);
    }
    // border rows
    for (int col = tid; col < ncols; col += WL_BLOCK)
    {
      const int ck = (kf < 0) ? col / npnt : kf;
      const int cc = (kf < 0) ? col - ck * npnt : col;
      const double* wc = win + (int64_t)col * NWIN;
      double yb[NBD];
#pragma unroll
      for (int b = 0; b < NBD; ++b)
      {
        double y = Bat(ck, nch + b, cc) - wc[BW + b];
#pragma unroll
        for (int q = 0; q < NBD; ++q)
          if (q < b)
            y -= bord[(int64_t)b * dimm + nch + q] * yb[q];
        y *= dinv[nch + b];
        yb[b] = y;
        Yb[b * LDY + ck * npm + cc] = y;
      }
    }
    fold(NBD, kf);
  };

  // ---- u_k = -A_k^-1 (B_k gamma) into w_k = Yb + k dimm (thread k, or the thread of kf) ----
  auto solve_u = [&](int kf) {
    double* wvec = Yb;
    for (int e = tid; e < 2 * dim; e += WL_BLOCK)
    {
      const int k = e / dim, q = e - k * dim;
      if (kf >= 0 && k != kf)
        continue;
      double t = 0.0;
      if (q == nch)
      {
        for (int c = 0; c < npnt; ++c)
          t += Bd[k * npm + c] * Gg[c];
      }
      else
      {
        const double* bv = Bv + ((int64_t)k * dimm + q) * 4;
        const int* pk = Bp + (int64_t)q * 4;
        t = bv[0] * Gg[0] + bv[1] * Gg[pk[0]] + bv[2] * Gg[pk[1]] + bv[3] * Gg[pk[2]];
      }
      wvec[k * dimm + q] = -t;
    }
    __syncthreads();
    if ((kf < 0 && tid < 2) || tid == kf)
    {
      double* w = wvec + tid * dimm;
      double wb[NBD];
      {
        // forward, chain: the last BW values stay in registers
        double wv[BW];
#pragma unroll
        for (int d = 0; d < BW; ++d)
          wv[d] = 0.0;
        for (int i = 0; i < nch; ++i)
        {
          double t = w[i];
#pragma unroll
          for (int d = 0; d < BW; ++d)
            t -= ((d + 1 <= i) ? band[(int64_t)i * LDB + d + 1] : 0.0) * wv[d];
          t *= dinv[i];
#pragma unroll
          for (int d = BW - 1; d > 0; --d)
            wv[d] = wv[d - 1];
          wv[0] = t;
          w[i] = t;
        }
      }
#pragma unroll
      for (int b = 0; b < NBD; ++b)
      {
        double t = w[nch + b];
        for (int q = 0; q < nch; ++q)
          t -= bord[(int64_t)b * dimm + q] * w[q];
#pragma unroll
        for (int q = 0; q < NBD; ++q)
          if (q < b)
            t -= bord[(int64_t)b * dimm + nch + q] * wb[q];
        wb[b] = t * dinv[nch + b];
      }
#pragma unroll
      for (int b = NBD - 1; b >= 0; --b)
      {
        double t = wb[b];
#pragma unroll
        for (int q = 0; q < NBD; ++q)
          if (q > b)
            t -= bord[(int64_t)q * dimm + nch + b] * wb[q];
        wb[b] = t * dinv[nch + b];
        w[nch + b] = wb[b];
      }
      {
        // backward, chain: wv[d] = w[i + 1 + d]
        double wv[BW];
#pragma unroll
        for (int d = 0; d < BW; ++d)
          wv[d] = 0.0;
        for (int i = nch - 1; i >= 0; --i)
        {
          double t = w[i];
#pragma unroll
          for (int d = 0; d < BW; ++d)
            t -= ((i + 1 + d < nch) ? band[(int64_t)(i + 1 + d) * LDB + d + 1] : 0.0) * wv[d];
#pragma unroll
          for (int b = 0; b < NBD; ++b)
            t -= bord[(int64_t)b * dimm + i] * wb[b];
          t *= dinv[i];
#pragma unroll
          for (int d = BW - 1; d > 0; --d)
            wv[d] = wv[d - 1];
          wv[0] = t;
          w[i] = t;
        }
      }
    }
    __syncthreads();
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

  // ---- Gaussian elimination with row pivoting of the (npnt [+1])^2 Schur system, with the rank-revealing threshold
  // of k_se_weaksym: the multiplier of a column without pivot is 0 ----
  {
    double cscale = 0.0;
    for (int64_t e = tid; e < (int64_t)dim_c * dim_c; e += WL_BLOCK)
    {
      const double v = Cg[(e / dim_c) * dcm + e % dim_c];
      if (!isfinite(v))
        status_local = 1;
      cscale = fmax(cscale, fabs(v));
    }
    cscale = block_max(cscale, red_v, tid);
    const double ptol = EQLB_WS_PIVOT_RTOL * cscale;
    int nr = 0; // rows used so far
    for (int c = 0; c < dim_c; ++c)
    {
      // first row of largest modulus among the rows not used yet
      double bv = -1.0;
      int br = 0x7fffffff;
      for (int r = nr + tid; r < dim_c; r += WL_BLOCK)
      {
        const double v = fabs(Cg[r * dcm + c]);
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
      __syncthreads();
      if ((tid & 63) == 0)
      {
        red_v[tid >> 6] = bv;
        red_i[tid >> 6] = br;
      }
      __syncthreads();
      bv = red_v[0];
      br = red_i[0];
#pragma unroll
      for (int w = 1; w < WL_BLOCK / 64; ++w)
        if (red_v[w] > bv || (red_v[w] == bv && red_i[w] < br))
        {
          bv = red_v[w];
          br = red_i[w];
        }
      if (!(bv > ptol))
      {
        if (tid == 0)
          pcol[c] = -1;
        continue;
      }
      if (!isfinite(bv))
        status_local = 1;
      if (br != nr)
      {
        for (int j = tid; j <= dim_c; j += WL_BLOCK)
        {
          double* x = (j < dim_c) ? Cg + nr * dcm + j : Rg + nr;
          double* y = (j < dim_c) ? Cg + br * dcm + j : Rg + br;
          const double t = *x;
          *x = *y;
          *y = t;
        }
        __syncthreads();
      }
      const double ip = 1.0 / Cg[nr * dcm + c];
      for (int r = nr + 1 + tid; r < dim_c; r += WL_BLOCK)
        fac[r] = Cg[r * dcm + c] * ip;
      __syncthreads();
      {
        // rows nr + 1 ... dim_c - 1, columns c ... dim_c - 1 and the right-hand side
        const int wdt = dim_c - c + 1;
        const int64_t nupd = (int64_t)(dim_c - nr - 1) * wdt;
        for (int64_t e = tid; e < nupd; e += WL_BLOCK)
        {
          const int r = nr + 1 + (int)(e / wdt), jj = (int)(e % wdt);
          const double f = fac[r];
          if (jj < wdt - 1)
            Cg[r * dcm + c + jj] -= f * Cg[nr * dcm + c + jj];
          else
            Rg[r] -= f * Rg[nr];
        }
      }
      if (tid == 0)
        pcol[c] = nr;
      ++nr;
      __syncthreads();
    }
    __syncthreads();
    if (tid == 0)
      ws_back_substitute(Cg, dcm, Rg, pcol, dim_c, Gg, &status_local);
    __syncthreads();
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
  for (int i = tid; i < n; i += WL_BLOCK)
  {
    const WsCell<K> c(a, te_table, vq_table, s0 + i, true, pt, i);
    int pos[NH];
    W::pos(pt, i, pos);
#pragma unroll
    for (int k = 0; k < 2; ++k)
    {
      const double* w = Yb + k * dimm;
      double ul[NH];
#pragma unroll
      for (int h = 0; h < NH; ++h)
        ul[h] = w[pos[h]];
      c.add_correction(ul, c.row(a.out, a.ncells, k));
    }
  }
  if (status_local)
    atomicOr(a.status, 2);
}

template <int K>
int launch_ws_large_t(const SeArgs& a, const WsLargeArgs& la, hipStream_t stream)
{
  hipLaunchKernelGGL((k_se_weaksym_large<K>), dim3((unsigned)a.npatch_total), dim3(WL_BLOCK), 0, stream, a, la);
  return (hipGetLastError() == hipSuccess) ? 0 : EQLB_ERR_DEVICE;
}
} // namespace

size_t large_patch_weaksym_ws_doubles(int k, int64_t ncells_of_patch)
{
  if (k == 2)
    return (size_t)WsLarge<2>(ncells_of_patch).total;
  if (k == 3)
    return (size_t)WsLarge<3>(ncells_of_patch).total;
  if (k == 4)
    return (size_t)WsLarge<4>(ncells_of_patch).total;
  return 0;
}

int launch_se_weaksym_large(int k, const SeArgs& a, const int32_t* off, const int64_t* wsoff, double* ws,
                            hipStream_t stream)
{
  if (a.npatch_total <= 0)
    return 0;
  const WsLargeArgs la{off, wsoff, ws};
  if (k == 2)
    return launch_ws_large_t<2>(a, la, stream);
  if (k == 3)
    return launch_ws_large_t<3>(a, la, stream);
  if (k == 4)
    return launch_ws_large_t<4>(a, la, stream);
  return EQLB_ERR_UNSUPPORTED;
}

} // namespace eqlb
