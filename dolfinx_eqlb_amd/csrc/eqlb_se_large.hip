// Vertex patches that do not fit one wavefront (more than 63 cells or more than 64 patch facets): one WORKGROUP per
// patch, the cells of the fan strided over its threads.
//
// Same formulation as se_patch_body (eqlb_se_body.h; numpy statement tests/proto_gpu_math.py): own-frame outward
// flux moments, element matrix and load from the reduced tensors TE / WQ of the handle's table buffer, the HB rule for
// inhomogeneous flux BCs with its 1e-7 skip, MODE 1 = the constrained-minimisation (EV) patch problem in the same
// reduced unknowns.  What differs is the mapping, so the result differs from the one-wave path by rounding only:
//   phase 1  one thread per cell: facet moments of hat*G, moments of hat*(f - div G)            (cell-local)
//   phase 2  jump moments on the plus facets: the neighbour's moments are read from the work space, not shuffled
//   phase 3  the zero-order recurrence t_i = t_{i-1} + R0_i + J0_{i-1} and the flux-BC shift delta, in fan order
//   phase 4  one thread per cell: particular solution, Te, Le, fixed (flux-BC) unknowns masked, the interior
//            unknowns of the cell condensed
//   phase 5  one thread per patch facet: block row of the reduced system in [d | x_0 | x_1 ... x_{nf-1}]
//   phase 6  one thread: the block-tridiagonal chain x_1 ... x_{nf-1} eliminated serially over the block rows with the
//            K + 1 right-hand sides [coupling to the border (d, x_0) | load], Schur complement of the border
//            (cyclic patches: x_{n-1} couples back to x_0; open fans: it does not), K x K solve
//   phase 7  one thread per cell: local unknowns, back-map to RT coefficients, the (cell, vertex) row into the slots
// The tables are read from global memory (L2 resident, 8 - 80 KB) and the per-patch work space lives in a global
// buffer sized at eqlb_se_set_boundary: no LDS, no per-patch size limit.  Threads of a workgroup hand data over through
// that buffer across __syncthreads().  Every sum runs in a fixed order: two calls give the same bits.
#include "eqlb_device_common.h"

namespace eqlb
{

namespace
{
constexpr int LP_BLOCK = 256;

// doubles per work-space row; a patch of n cells owns n + 2 rows: row i holds the data of cell i and of facet E_i
// (i <= n), the last row the patch header
template <int K>
struct LargeRow
{
  static constexpr int KB = K - 1, NADD = (K - 1) * (K - 2) / 2, NQ = nq_of(K);
  static constexpr int NH = 1 + 2 * KB + NADD, NC = 1 + 2 * KB;
  static constexpr int GM = 0, GP = GM + K, BM = GP + K, BP = BM + K, RQ = BP + K, LEG = RQ + NQ, JV = LEG + NH;
  static constexpr int SR0 = JV + K, T = SR0 + 1, MUM = T + 1, MUP = MUM + K, M = MUP + K, L = M + NC * NC;
  static constexpr int CA = L + NC, LA = CA + NC * NADD;
  static constexpr int FA = LA + NADD, FC = FA + KB * KB, FE = FC + KB * KB, FW = FE + KB * K;
  static constexpr int END = FW + KB * (K + 1);
  static constexpr int STRIDE = END + (END & 1);
  // header row
  static constexpr int H_DELTA = 0, H_XB = 1; // xb: [d | x_0] (K doubles)
  static_assert(H_XB + K <= STRIDE, "header row");
};

// y = (rev ? B : I) x with the binomial matrix B of bcoef
template <int K>
__device__ __forceinline__ void reversal(const double (&x)[K], const bool rev, double (&y)[K])
{
#pragma unroll
  for (int j = 0; j < K; ++j)
  {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c <= j; ++c)
      s += bcoef(j, c) * x[c];
    y[j] = rev ? s : x[j];
  }
}

// inverse of a symmetric positive definite N x N matrix (Gauss-Jordan without pivoting); false: a pivot is not positive
template <int N>
__device__ __forceinline__ bool inv_spd(double (&W)[N][N], double (&Ai)[N][N])
{
  bool ok = true;
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j)
      Ai[i][j] = (i == j) ? 1.0 : 0.0;
#pragma unroll
  for (int p = 0; p < N; ++p)
  {
    const double piv = W[p][p];
    ok = ok && (piv > 0.0);
    const double r = 1.0 / (piv > 0.0 ? piv : 1.0);
#pragma unroll
    for (int j = 0; j < N; ++j)
    {
      W[p][j] *= r;
      Ai[p][j] *= r;
    }
#pragma unroll
    for (int i = 0; i < N; ++i)
    {
      if (i == p)
        continue;
      const double f = W[i][p];
#pragma unroll
      for (int j = 0; j < N; ++j)
      {
        W[i][j] -= f * W[p][j];
        Ai[i][j] -= f * Ai[p][j];
      }
    }
  }
  return ok;
}

struct LargeArgs
{
  const int32_t* off; // [npatch + 1] first lane slot of the patch in slot_cell / slot_info (CSR)
  double* ws;         // work space, (nslots + 2 npatch) rows
};

template <int K, int DEG, int MODE>
__global__ void __launch_bounds__(LP_BLOCK) k_se_patch_large(const SeArgs a, const LargeArgs la)
{
  using Z = Sizes<K, DEG, 64>;
  using W = LargeRow<K>;
  constexpr int KB = Z::KB, NADD = Z::NADD, NDIV = Z::NDIV, NRT = Z::NRT, ND = Z::ND, NQ = Z::NQ;
  constexpr int NCOL = Z::NCOL, NH = Z::NH, NC = W::NC, NTES = Z::NTES, NCOLS = Z::NCOLS;
  constexpr int KB1 = (KB > 0) ? KB : 1, NADD1 = (NADD > 0) ? NADD : 1; // array extents
  const double* tF = a.tables + Z::NS;
  const double* tHt = tF + Z::NF;
  const double* tDt = tHt + Z::NHT;
  const double* tTE = a.tables + Z::OFF_TE;
  const double* tWQ = tTE + Z::NTET;
  const double* tHB = tWQ + Z::NWQT;
  const double* tHG = a.tables + Z::OFF_HG;
  const double* tWG = tHG + Z::NHG;
  (void)tF;
  (void)tDt;
  (void)tHG;
  (void)tWG;

  const int patch = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t s0 = la.off[patch];
  const int n = (int)(la.off[patch + 1] - s0);
  const uint8_t flag0 = a.pflag[patch];
  const uint8_t flag = a.pflag[(int64_t)a.rhs * a.npatch_total + patch];
  const bool interior = (flag0 & PFLAG_INTERIOR) != 0;
  const bool bc0 = (flag & PFLAG_BC0) != 0, bcn = (flag & PFLAG_BCN) != 0;
  const bool d_fixed = bc0 || bcn;
  const int nf = interior ? n : n + 1;
  double* const wsp = la.ws + (s0 + 2 * (int64_t)patch) * W::STRIDE;
  auto row = [&](int i) -> double* { return wsp + (int64_t)i * W::STRIDE; };
  double* const hdr = row(n + 1);
  const int r = a.rhs;
  bool bad = false;

  // ---- phase 1: cell-local integrals ----
  for (int i = tid; i < n; i += LP_BLOCK)
  {
    const int32_t cell = a.slot_cell[s0 + i];
    const uint32_t info = a.slot_info[s0 + i];
    const int fm = (info >> INFO_FM_SHIFT) & 3, fp = (info >> INFO_FP_SHIFT) & 3, ln = (info >> INFO_LN_SHIFT) & 3;
    const bool rev_m = (info & INFO_REV_M) != 0;
    const int ci = combo_index(fm, fp, rev_m);
    (void)ci;
    const double* Jp = a.cellJ + 4 * (int64_t)cell;
    const double J00 = Jp[0], J01 = Jp[1], J10 = Jp[2], J11 = Jp[3];
    const double detJ = J00 * J11 - J01 * J10;
    const double sgn = (detJ > 0.0) ? 1.0 : -1.0;
    const double pf_m = (fm == 1) ? sgn : -sgn, pf_p = (fp == 1) ? sgn : -sgn;
    const double a00 = J11, a01 = -J01, a10 = -J10, a11 = J00; // adj = detJ * K
    const double* gd = a.flux_dg + ((int64_t)a.rhs_in * a.ncells + cell) * (ND * 2);
    const double* fd_ = a.rhs_dg + ((int64_t)a.rhs_in * a.ncells + cell) * ND;
    const double* tH = tHt + ln * Z::HROW;
    double gm[K], gpv[K], Rq[NQ];
#pragma unroll
    for (int j = 0; j < K; ++j)
      gm[j] = gpv[j] = 0.0;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      Rq[q] = 0.0;
    double* w = row(i);
    if constexpr (MODE == 1)
    {
      double LeG[NH];
#pragma unroll
      for (int h = 0; h < NH; ++h)
        LeG[h] = 0.0;
      const double* wg = tWG + ci * NH * ND * 2;
      const double dh0 = (ln == 0) ? -1.0 : ((ln == 1) ? 1.0 : 0.0);
      const double dh1 = (ln == 0) ? -1.0 : ((ln == 2) ? 1.0 : 0.0);
#pragma unroll
      for (int e = 0; e < ND; ++e)
      {
        const double gx = gd[2 * e], gy = gd[2 * e + 1];
        const double fd = detJ * fd_[e];
        const double gg = dh0 * (a00 * gx + a01 * gy) + dh1 * (a10 * gx + a11 * gy);
        const double jt0 = J00 * gx + J10 * gy, jt1 = J01 * gx + J11 * gy; // J^T G_e
#pragma unroll
        for (int q = 0; q < NQ; ++q)
          Rq[q] = __builtin_fma(gg, tHG[e * NQ + q], __builtin_fma(fd, tH[e * NQ + q], Rq[q]));
#pragma unroll
        for (int h = 0; h < NH; ++h)
          LeG[h] = __builtin_fma(wg[(h * ND + e) * 2 + 1], jt1, __builtin_fma(wg[(h * ND + e) * 2], jt0, LeG[h]));
      }
#pragma unroll
      for (int h = 0; h < NH; ++h)
        w[W::LEG + h] = LeG[h];
    }
    else
    {
      const double nmx = (fm == 2) ? 0.0 : -1.0, nmy = (fm == 0) ? -1.0 : ((fm == 1) ? 0.0 : 1.0);
      const double npx = (fp == 2) ? 0.0 : -1.0, npy = (fp == 0) ? -1.0 : ((fp == 1) ? 0.0 : 1.0);
      const double num0 = a00 * nmx + a10 * nmy, num1 = a01 * nmx + a11 * nmy;
      const double nup0 = a00 * npx + a10 * npy, nup1 = a01 * npx + a11 * npy;
      const double* tF_m = tF + (fm * 3 + ln) * ND * K;
      const double* tF_p = tF + (fp * 3 + ln) * ND * K;
      const double* tD = tDt + ln * ND * 2 * NQ;
      // (RT_4 with DG_3 data: the unrolled loop keeps 10 x 30 table reads in flight and spills)
      constexpr int UNR = (ND > 6) ? 1 : ND;
#pragma unroll UNR
      for (int e = 0; e < ND; ++e)
      {
        const double gx = gd[2 * e], gy = gd[2 * e + 1];
        const double gnm = gx * num0 + gy * num1, gnp = gx * nup0 + gy * nup1;
        const double gh0 = a00 * gx + a01 * gy, gh1 = a10 * gx + a11 * gy; // (adj G_e)_X
        const double fd = detJ * fd_[e];
#pragma unroll
        for (int j = 0; j < K; ++j)
        {
          gm[j] += tF_m[e * K + j] * gnm;
          gpv[j] += tF_p[e * K + j] * gnp;
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q)
          Rq[q] = __builtin_fma(-gh1, tD[(e * 2 + 1) * NQ + q],
                                __builtin_fma(-gh0, tD[(e * 2 + 0) * NQ + q], __builtin_fma(fd, tH[e * NQ + q], Rq[q])));
      }
#pragma unroll
      for (int j = 0; j < K; ++j)
      {
        gm[j] *= pf_m;
        gpv[j] *= pf_p;
      }
    }
    // prescribed outward moments of sigma_a on flux-BC end facets: pf * HB[f][ln] b - (hat_a G); |b| < 1e-7: skipped
    double bnd_m[K], bnd_p[K];
#pragma unroll
    for (int j = 0; j < K; ++j)
    {
      bnd_m[j] = -gm[j];
      bnd_p[j] = -gpv[j];
    }
    if (a.bvals != nullptr && d_fixed)
    {
      const bool at0 = bc0 && i == 0, atn = bcn && i == n - 1;
      if (at0 || atn)
      {
        const double* bv = a.bvals + ((int64_t)r * a.ncells + cell) * NRT;
#pragma unroll
        for (int side = 0; side < 2; ++side)
        {
          if (!(side == 0 ? at0 : atn))
            continue;
          const int fb = side == 0 ? fm : fp;
          const double pfb = side == 0 ? pf_m : pf_p;
          double bg[K];
          bool allzero = true;
#pragma unroll
          for (int j = 0; j < K; ++j)
          {
            bg[j] = bv[fb * K + j];
            allzero = allzero && (fabs(bg[j]) < 1e-7);
          }
          if (!allzero)
          {
            const double* hb = tHB + (fb * 3 + ln) * K * K;
#pragma unroll
            for (int ii = 0; ii < K; ++ii)
            {
              double s = 0.0;
#pragma unroll
              for (int j = 0; j < K; ++j)
                s += hb[ii * K + j] * bg[j];
              if (side == 0)
                bnd_m[ii] += pfb * s;
              else
                bnd_p[ii] += pfb * s;
            }
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < K; ++j)
    {
      w[W::GM + j] = gm[j];
      w[W::GP + j] = gpv[j];
      w[W::BM + j] = bnd_m[j];
      w[W::BP + j] = bnd_p[j];
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      w[W::RQ + q] = Rq[q];
    w[W::SR0] = sgn * Rq[0];
  }
  __syncthreads();

  // ---- phase 2: jump moments on the plus facet (owner frame) ----
  for (int i = tid; i < n; i += LP_BLOCK)
  {
    const uint32_t info = a.slot_info[s0 + i];
    const bool rev_p = (info & INFO_REV_P) != 0;
    const bool has_next = interior || i < n - 1;
    const int next = (i + 1 < n) ? i + 1 : (interior ? 0 : i);
    double* w = row(i);
    const double* wn = row(next);
    double gmn[K], gt[K];
#pragma unroll
    for (int j = 0; j < K; ++j)
      gmn[j] = wn[W::GM + j];
    reversal<K>(gmn, rev_p, gt);
#pragma unroll
    for (int j = 0; j < K; ++j)
      w[W::JV + j] = has_next ? w[W::GP + j] + gt[j] : 0.0;
  }
  __syncthreads();

  // ---- phase 3: zero-order recurrence in fan order, shift delta of the flux-BC configurations ----
  if (tid == 0)
  {
    double t = 0.0;
    for (int i = 0; i < n; ++i)
    {
      const bool has_prev = interior || i > 0;
      const int prev = (i > 0) ? i - 1 : n - 1;
      t += row(i)[W::SR0] + (has_prev ? row(prev)[W::JV] : 0.0);
      row(i)[W::T] = t;
    }
    double delta = 0.0;
    if (d_fixed)
      delta = bc0 ? -row(0)[W::BM] : (row(n - 1)[W::BP] - t);
    hdr[W::H_DELTA] = delta;
  }
  __syncthreads();

  // ---- phase 4: particular solution, element matrix and load, interior unknowns condensed ----
  const double delta = hdr[W::H_DELTA];
  for (int i = tid; i < n; i += LP_BLOCK)
  {
    const int32_t cell = a.slot_cell[s0 + i];
    const uint32_t info = a.slot_info[s0 + i];
    const int fm = (info >> INFO_FM_SHIFT) & 3, fp = (info >> INFO_FP_SHIFT) & 3;
    const bool rev_m = (info & INFO_REV_M) != 0;
    const int ci = combo_index(fm, fp, rev_m);
    const double* Jp = a.cellJ + 4 * (int64_t)cell;
    const double J00 = Jp[0], J01 = Jp[1], J10 = Jp[2], J11 = Jp[3];
    const double detJ = J00 * J11 - J01 * J10;
    const double sgn = (detJ > 0.0) ? 1.0 : -1.0;
    const bool has_prev = interior || i > 0;
    const int prev = (i > 0) ? i - 1 : n - 1;
    double* w = row(i);
    const double* wp = row(prev);
    double mu_m[K], mu_p[K];
    mu_p[0] = w[W::T] + delta;
#pragma unroll
    for (int j = 1; j < K; ++j)
      mu_p[j] = (bcn && i == n - 1) ? w[W::BP + j] : 0.0;
    if (has_prev)
    {
      double vprev[K], vt[K];
      vprev[0] = wp[W::T] + delta + wp[W::JV];
#pragma unroll
      for (int j = 1; j < K; ++j)
        vprev[j] = ((bcn && prev == n - 1) ? wp[W::BP + j] : 0.0) + wp[W::JV + j];
      reversal<K>(vprev, rev_m, vt);
#pragma unroll
      for (int j = 0; j < K; ++j)
        mu_m[j] = -vt[j];
    }
    else
    {
      mu_m[0] = -delta;
#pragma unroll
      for (int j = 1; j < K; ++j)
        mu_m[j] = bc0 ? w[W::BM + j] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < K; ++j)
    {
      w[W::MUM + j] = mu_m[j];
      w[W::MUP + j] = mu_p[j];
    }

    // Te = sum_x g_x TE[ci][x], Le = -sum_x g_x WQ[ci][x] [mu_m; mu_p; sgn c_div], g = J^T J / |detJ|
    const double ia = 1.0 / fabs(detJ);
    const double g0 = (J00 * J00 + J10 * J10) * ia, g1 = (J00 * J01 + J10 * J11) * ia, g2 = (J01 * J01 + J11 * J11) * ia;
    // unknowns fixed by a flux BC: zero rows and columns here, identity rows in phases 5 / 6
    double mk[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h)
      mk[h] = 1.0;
    if (d_fixed)
      mk[0] = 0.0;
#pragma unroll
    for (int aa = 0; aa < KB; ++aa)
    {
      if (bc0 && i == 0)
        mk[1 + aa] = 0.0;
      if (bcn && i == n - 1)
        mk[1 + KB + aa] = 0.0;
    }
    double Te[NH][NH], Le[NH];
    const double* te = tTE + ci * 3 * NTES;
#pragma unroll
    for (int h = 0; h < NH; ++h)
#pragma unroll
      for (int g = 0; g <= h; ++g)
      {
        const int e = h * (h + 1) / 2 + g;
        const double v = (g0 * te[e] + g1 * te[NTES + e] + g2 * te[2 * NTES + e]) * mk[h] * mk[g];
        Te[h][g] = v;
        Te[g][h] = v;
      }
    {
      double full[NCOL];
#pragma unroll
      for (int j = 0; j < K; ++j)
      {
        full[j] = mu_m[j];
        full[K + j] = mu_p[j];
      }
#pragma unroll
      for (int q = 0; q < NDIV; ++q)
        full[2 * K + q] = sgn * w[W::RQ + 1 + q];
      const double* wq = tWQ + ci * 3 * NH * NCOLS;
#pragma unroll
      for (int h = 0; h < NH; ++h)
      {
        double q0 = 0.0, q1 = 0.0, q2 = 0.0;
#pragma unroll
        for (int c = 0; c < NCOL; ++c)
        {
          q0 += wq[h * NCOLS + c] * full[c];
          q1 += wq[(NH + h) * NCOLS + c] * full[c];
          q2 += wq[(2 * NH + h) * NCOLS + c] * full[c];
        }
        double v = -(g0 * q0 + g1 * q1 + g2 * q2);
        if constexpr (MODE == 1)
          v += w[W::LEG + h];
        Le[h] = v * mk[h];
      }
    }
    // condense the interior unknowns ua: Taa X = [Tac | Le_a]
    double X[NADD1][NC + 1];
    (void)X;
    if constexpr (NADD > 0)
    {
      double Taa[NADD][NADD], Tai[NADD][NADD];
#pragma unroll
      for (int p = 0; p < NADD; ++p)
#pragma unroll
        for (int q = 0; q < NADD; ++q)
          Taa[p][q] = Te[NC + p][NC + q];
      if (!inv_spd<NADD>(Taa, Tai))
        bad = true;
#pragma unroll
      for (int p = 0; p < NADD; ++p)
#pragma unroll
        for (int c = 0; c <= NC; ++c)
        {
          double s = 0.0;
#pragma unroll
          for (int q = 0; q < NADD; ++q)
            s += Tai[p][q] * ((c < NC) ? Te[NC + q][c] : Le[NC + q]);
          X[p][c] = s;
        }
#pragma unroll
      for (int h = 0; h < NC; ++h)
#pragma unroll
        for (int q = 0; q < NADD; ++q)
          w[W::CA + h * NADD + q] = X[q][h];
#pragma unroll
      for (int q = 0; q < NADD; ++q)
        w[W::LA + q] = X[q][NC];
    }
#pragma unroll
    for (int h = 0; h < NC; ++h)
    {
#pragma unroll
      for (int g = 0; g < NC; ++g)
      {
        double v = Te[h][g];
        if constexpr (NADD > 0)
        {
#pragma unroll
          for (int q = 0; q < NADD; ++q)
            v -= Te[h][NC + q] * X[q][g];
        }
        w[W::M + h * NC + g] = v;
      }
      double v = Le[h];
      if constexpr (NADD > 0)
      {
#pragma unroll
        for (int q = 0; q < NADD; ++q)
          v -= Te[h][NC + q] * X[q][NC];
      }
      w[W::L + h] = v;
    }
  }
  __syncthreads();

  // ---- phase 5: block rows of the reduced system, one thread per patch facet ----
  if constexpr (KB > 0)
  {
    for (int f = tid; f < nf; f += LP_BLOCK)
    {
      const bool own = f < n;
      const int pc = (f > 0) ? f - 1 : (interior ? n - 1 : -1);
      const bool fixed_f = (bc0 && f == 0) || (bcn && f == n);
      const double* mo = row(own ? f : 0) + W::M;
      const double* lo = row(own ? f : 0) + W::L;
      const double* mp = row(pc >= 0 ? pc : 0) + W::M;
      const double* lp = row(pc >= 0 ? pc : 0) + W::L;
      const double so = own ? 1.0 : 0.0, sp = (pc >= 0) ? 1.0 : 0.0;
      double* w = row(f);
#pragma unroll
      for (int aa = 0; aa < KB; ++aa)
      {
#pragma unroll
        for (int bb = 0; bb < KB; ++bb)
        {
          w[W::FA + aa * KB + bb] = so * mo[(1 + aa) * NC + 1 + bb] + sp * mp[(1 + KB + aa) * NC + 1 + KB + bb]
                                    + ((fixed_f && aa == bb) ? 1.0 : 0.0);
          w[W::FC + aa * KB + bb] = so * mo[(1 + aa) * NC + 1 + KB + bb];
          // coupling of x_f with x_0: facet 1 through cell 0, facet n - 1 of a ring through cell n - 1
          double e0 = 0.0;
          if (f == 1)
            e0 += row(0)[W::M + (1 + bb) * NC + 1 + KB + aa];
          if (interior && f == n - 1)
            e0 += mo[(1 + aa) * NC + 1 + KB + bb];
          w[W::FE + aa * K + 1 + bb] = e0;
          w[W::FW + aa * (K + 1) + 1 + bb] = e0;
        }
        const double bd = so * mo[(1 + aa) * NC] + sp * mp[(1 + KB + aa) * NC];
        w[W::FE + aa * K] = bd;
        w[W::FW + aa * (K + 1)] = bd;
        w[W::FW + aa * (K + 1) + K] = so * lo[1 + aa] + sp * lp[1 + KB + aa];
      }
    }
    __syncthreads();
  }

  // ---- phase 6: serial elimination over the block rows ----
  if (tid == 0)
  {
    double add = d_fixed ? 1.0 : 0.0, rd = 0.0;
    for (int i = 0; i < n; ++i)
    {
      add += row(i)[W::M];
      rd += row(i)[W::L];
    }
    if constexpr (KB == 0)
    {
      if (!(add > 0.0))
        bad = true;
      hdr[W::H_XB] = d_fixed ? 0.0 : rd / add; // se/PatchData.hpp:589
    }
    else
    {
      const int m = nf - 1; // chain rows 1 .. m
      double Dinv[KB1][KB1], Wp[KB1][K + 1];
      // forward
      for (int j = 1; j <= m; ++j)
      {
        double* w = row(j);
        double D[KB1][KB1], Wj[KB1][K + 1];
#pragma unroll
        for (int aa = 0; aa < KB; ++aa)
        {
#pragma unroll
          for (int bb = 0; bb < KB; ++bb)
            D[aa][bb] = w[W::FA + aa * KB + bb];
#pragma unroll
          for (int c = 0; c <= K; ++c)
            Wj[aa][c] = w[W::FW + aa * (K + 1) + c];
        }
        if (j > 1)
        {
          const double* cp = row(j - 1) + W::FC; // A_{j-1,j} = C_{j-1}, A_{j,j-1} = C_{j-1}^T
          double C[KB1][KB1], Lj[KB1][KB1];
#pragma unroll
          for (int aa = 0; aa < KB; ++aa)
#pragma unroll
            for (int bb = 0; bb < KB; ++bb)
              C[aa][bb] = cp[aa * KB + bb];
#pragma unroll
          for (int aa = 0; aa < KB; ++aa)
#pragma unroll
            for (int bb = 0; bb < KB; ++bb)
            {
              double s = 0.0;
#pragma unroll
              for (int cc = 0; cc < KB; ++cc)
                s += C[cc][aa] * Dinv[cc][bb];
              Lj[aa][bb] = s;
            }
#pragma unroll
          for (int aa = 0; aa < KB; ++aa)
          {
#pragma unroll
            for (int bb = 0; bb < KB; ++bb)
            {
              double s = 0.0;
#pragma unroll
              for (int cc = 0; cc < KB; ++cc)
                s += Lj[aa][cc] * C[cc][bb];
              D[aa][bb] -= s;
            }
#pragma unroll
            for (int c = 0; c <= K; ++c)
            {
              double s = 0.0;
#pragma unroll
              for (int cc = 0; cc < KB; ++cc)
                s += Lj[aa][cc] * Wp[cc][c];
              Wj[aa][c] -= s;
            }
          }
        }
        if (!inv_spd<KB1>(D, Dinv))
          bad = true;
#pragma unroll
        for (int aa = 0; aa < KB; ++aa)
        {
#pragma unroll
          for (int bb = 0; bb < KB; ++bb)
            w[W::FA + aa * KB + bb] = Dinv[aa][bb];
#pragma unroll
          for (int c = 0; c <= K; ++c)
          {
            w[W::FW + aa * (K + 1) + c] = Wj[aa][c];
            Wp[aa][c] = Wj[aa][c];
          }
        }
      }
      // border [d | x_0]: matrix and load
      double S[K][K], rb[K];
      {
        const double* w0 = row(0);
#pragma unroll
        for (int p = 0; p < K; ++p)
#pragma unroll
          for (int q = 0; q < K; ++q)
            S[p][q] = 0.0;
        S[0][0] = add;
        rb[0] = rd;
#pragma unroll
        for (int aa = 0; aa < KB; ++aa)
        {
          S[0][1 + aa] = S[1 + aa][0] = w0[W::FE + aa * K];
          rb[1 + aa] = w0[W::FW + aa * (K + 1) + K];
#pragma unroll
          for (int bb = 0; bb < KB; ++bb)
            S[1 + aa][1 + bb] = w0[W::FA + aa * KB + bb];
        }
      }
      // backward: Z_j = chain^-1 [E | r] row j, Schur complement of the border
      double Zn[KB1][K + 1];
      for (int j = m; j >= 1; --j)
      {
        double* w = row(j);
        double Wj[KB1][K + 1], Zj[KB1][K + 1];
#pragma unroll
        for (int aa = 0; aa < KB; ++aa)
#pragma unroll
          for (int c = 0; c <= K; ++c)
            Wj[aa][c] = w[W::FW + aa * (K + 1) + c];
        if (j < m)
        {
#pragma unroll
          for (int aa = 0; aa < KB; ++aa)
#pragma unroll
            for (int c = 0; c <= K; ++c)
            {
              double s = 0.0;
#pragma unroll
              for (int cc = 0; cc < KB; ++cc)
                s += w[W::FC + aa * KB + cc] * Zn[cc][c];
              Wj[aa][c] -= s;
            }
        }
#pragma unroll
        for (int aa = 0; aa < KB; ++aa)
#pragma unroll
          for (int c = 0; c <= K; ++c)
          {
            double s = 0.0;
#pragma unroll
            for (int cc = 0; cc < KB; ++cc)
              s += w[W::FA + aa * KB + cc] * Wj[cc][c];
            Zj[aa][c] = s;
          }
#pragma unroll
        for (int aa = 0; aa < KB; ++aa)
#pragma unroll
          for (int c = 0; c <= K; ++c)
          {
            w[W::FW + aa * (K + 1) + c] = Zj[aa][c];
            Zn[aa][c] = Zj[aa][c];
          }
#pragma unroll
        for (int p = 0; p < K; ++p)
        {
#pragma unroll
          for (int q = 0; q < K; ++q)
          {
            double s = 0.0;
#pragma unroll
            for (int aa = 0; aa < KB; ++aa)
              s += w[W::FE + aa * K + p] * Zj[aa][q];
            S[p][q] -= s;
          }
          double s = 0.0;
#pragma unroll
          for (int aa = 0; aa < KB; ++aa)
            s += w[W::FE + aa * K + p] * Zj[aa][K];
          rb[p] -= s;
        }
      }
      double Si[K][K];
      if (!inv_spd<K>(S, Si))
        bad = true;
#pragma unroll
      for (int p = 0; p < K; ++p)
      {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < K; ++q)
          s += Si[p][q] * rb[q];
        hdr[W::H_XB + p] = s;
      }
    }
  }
  __syncthreads();

  // ---- phase 7: local unknowns, back-map to RT coefficients, slot row ----
  double xb[K];
#pragma unroll
  for (int p = 0; p < K; ++p)
    xb[p] = hdr[W::H_XB + p];
  for (int i = tid; i < n; i += LP_BLOCK)
  {
    const int32_t cell = a.slot_cell[s0 + i];
    const uint32_t info = a.slot_info[s0 + i];
    const int fm = (info >> INFO_FM_SHIFT) & 3, fp = (info >> INFO_FP_SHIFT) & 3, ln = (info >> INFO_LN_SHIFT) & 3;
    const bool rev_m = (info & INFO_REV_M) != 0;
    const double* Jp = a.cellJ + 4 * (int64_t)cell;
    const double detJ = Jp[0] * Jp[3] - Jp[1] * Jp[2];
    const double sgn = (detJ > 0.0) ? 1.0 : -1.0;
    const double pf_m = (fm == 1) ? sgn : -sgn, pf_p = (fp == 1) ? sgn : -sgn;
    const int fi_p = interior ? ((i + 1 < n) ? i + 1 : 0) : i + 1;
    const double* w = row(i);
    double ul[NH];
    ul[0] = xb[0];
    if constexpr (KB > 0)
    {
      // x_f = Z_f[:, K] - Z_f[:, :K] [d | x_0] (f >= 1), x_0 from the border
#pragma unroll
      for (int side = 0; side < 2; ++side)
      {
        const int f = side == 0 ? i : fi_p;
        const double* z = row(f) + W::FW;
#pragma unroll
        for (int aa = 0; aa < KB; ++aa)
        {
          double v = z[aa * (K + 1) + K];
#pragma unroll
          for (int q = 0; q < K; ++q)
            v -= z[aa * (K + 1) + q] * xb[q];
          ul[1 + side * KB + aa] = (f == 0) ? xb[1 + aa] : v;
        }
      }
    }
    if constexpr (NADD > 0)
    {
#pragma unroll
      for (int q = 0; q < NADD; ++q)
      {
        double v = w[W::LA + q];
#pragma unroll
        for (int h = 0; h < NC; ++h)
          v -= w[W::CA + h * NADD + q] * ul[h];
        ul[NC + q] = v;
      }
    }
    // own-frame moments: mu_m -= Bm [d; um], mu_p += [d; up]
    double uk[K], ut[K], ym[K], yp[K];
#pragma unroll
    for (int c = 0; c < K; ++c)
      uk[c] = ul[c];
    reversal<K>(uk, rev_m, ut);
#pragma unroll
    for (int j = 0; j < K; ++j)
    {
      ym[j] = w[W::MUM + j] - ut[j];
      yp[j] = w[W::MUP + j] + ((j == 0) ? ul[0] : ul[KB + j]);
    }
    double* o = a.out + (((int64_t)a.rhs_out * a.ncells + cell) * 3 + ln) * NRT;
#pragma unroll
    for (int e = 0; e < 3 * K; ++e)
    {
      const int fe = e / K, j = e % K;
      o[e] = (fe == fm) ? pf_m * ym[j] : ((fe == fp) ? pf_p * yp[j] : 0.0);
    }
#pragma unroll
    for (int q = 0; q < NDIV; ++q)
      o[3 * K + q] = w[W::RQ + 1 + q];
#pragma unroll
    for (int q = 0; q < NADD; ++q)
      o[3 * K + NDIV + q] = sgn * ul[1 + 2 * KB + q];
  }

  if (bad)
    atomicOr(a.status, 1);
}

template <int K, int DEG, int MODE>
int launch_large_t(const SeArgs& a, const LargeArgs& la, hipStream_t stream)
{
  hipLaunchKernelGGL((k_se_patch_large<K, DEG, MODE>), dim3((unsigned)a.npatch_total), dim3(LP_BLOCK), 0, stream, a, la);
  return (hipGetLastError() == hipSuccess) ? 0 : EQLB_ERR_DEVICE;
}
} // namespace

size_t large_patch_ws_doubles(int k, int64_t nslots, int64_t npatch)
{
  const int stride = (k == 1) ? LargeRow<1>::STRIDE
                              : ((k == 2) ? LargeRow<2>::STRIDE : ((k == 3) ? LargeRow<3>::STRIDE : LargeRow<4>::STRIDE));
  return (size_t)(nslots + 2 * npatch) * stride;
}

int launch_se_patch_large(int k, int deg, int mode, const SeArgs& a, const int32_t* off, double* ws, hipStream_t stream)
{
  if (a.npatch_total <= 0)
    return 0;
  const LargeArgs la{off, ws};
#define EQLB_LARGE_CASE(KK, DD)                                                                     \
  if (k == KK && deg == DD)                                                                         \
  {                                                                                                 \
    if (mode == 0)                                                                                  \
      return launch_large_t<KK, DD, 0>(a, la, stream);                                              \
    if constexpr (KK <= 3)                                                                          \
      return launch_large_t<KK, DD, 1>(a, la, stream);                                              \
    return EQLB_ERR_UNSUPPORTED;                                                                    \
  }
  EQLB_LARGE_CASE(1, 0)
  EQLB_LARGE_CASE(2, 1)
  EQLB_LARGE_CASE(2, 0)
  EQLB_LARGE_CASE(3, 2)
  EQLB_LARGE_CASE(3, 1)
  EQLB_LARGE_CASE(3, 0)
  EQLB_LARGE_CASE(4, 3)
  EQLB_LARGE_CASE(4, 2)
  EQLB_LARGE_CASE(4, 1)
  EQLB_LARGE_CASE(4, 0)
#undef EQLB_LARGE_CASE
  return EQLB_ERR_UNSUPPORTED;
}

} // namespace eqlb
