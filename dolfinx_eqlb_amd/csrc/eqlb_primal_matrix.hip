// The P_p Poisson and [P_p]^2 elasticity operators AS CSR ON THE DEVICE: eqlb_primal_matrix_*, eqlb_elasticity_matrix_*
// and eqlb_csr_apply of include/eqlb.h.  The rule is stated there and, as numpy, in dolfinx_eqlb_amd/lsolver/primal.py
// (PoissonOperator.matrix, ElasticityOperator.matrix, csr_apply); indptr, indices and values reproduce it bit for bit.
// The solves, the hierarchy and the exact coarse solve do not use the matrix: they keep the matrix-free product.
//
// PATTERN (once per handle, kept in it: MatrixPattern of eqlb_primal_handle.h).  The scalar pattern, the distinct pairs
// (d, d') of DOFs with a common cell:
//   k_matrix_keys     one thread per (cell, i, j): the key d ndofs + d' of the pair - ncells nd_p^2 keys
//   radix_sort_keys   rocprim, on the bits ndofs^2 - 1 needs
//   unique            rocprim, the distinct keys in their order and their count; the call waits once for the count
//   k_matrix_rows     one thread per pair: row and column of the pair, and the offset of every row that begins at it
// No patch-shape formula, no per-thread buffer and no atomic: a vertex of any valence, a pinched vertex, several
// components and a node without a cell (an empty row) need nothing of their own.
// WORK SPACE of the build: two key arrays of ncells nd_p^2 * 8 bytes and rocprim's temporary storage, freed when the
// pattern stands; kept are 8 (ndofs + 1) + 8 snnz bytes.  The key list at P_4 is ncells * 225 keys: 3.6 GB for the two
// arrays at 1M cells (P_1: 144 MB, P_2: 576 MB).  MatrixPattern::peak_bytes has the figure of a handle.
//
// FILL  k_matrix_fill<BS, P, RX, VX>: one thread per pair.  It walks the slot list of the row's DOF (the order of the
//   owner sum), finds the local index of the column's DOF in each cell by matching ids, forms the BS x BS entries of the
//   cell from cellJ and the handle's coefficients and adds them from the first cell on.  Nothing is staged per cell, so
//   the values follow set_reaction, set_shear, set_diffusion, set_dirichlet and a new kappa or pi_1 without a new
//   pattern.  RX: the reaction term (Mass<P> is read with it only); VX: the diffusion tensor (BS = 1) or the shear
//   modulus (BS = 2).  The tables are read from constant memory by (i, j).
// PRODUCT  k_csr_apply<G>: one row per thread, the sum in ascending positions as the statement has it; where a bundle
//   of G neighbouring rows holds a long one, the G lanes sum the rows of the bundle together, in the same order (the
//   kernel says how).  G and the length are build parameters (eqlb_tuning.h), set by tools/matrix_time.py.
#include "eqlb_device_common.h"
#include "eqlb_matrix_plan.h"
#include "eqlb_primal_handle.h" // MatrixPattern, MatrixView; eqlb_primal_common.h: SpaceArgs, slot_range
#include "eqlb_tables_gen.h"

#include <cstring> // (rocprim's texture iterator calls memset)
#include <rocprim/rocprim.hpp>

namespace eqlb
{
namespace
{
constexpr int MX_THREADS = PS_THREADS;
constexpr int CSR_GROUP = EQLB_CSR_GROUP, CSR_GROUP_MIN = EQLB_CSR_GROUP_MIN; // (eqlb_tuning.h)
constexpr int MX_MAXBLOCKS = 2048; // blocks of a grid-stride kernel over pairs or keys; the product: stream_blocks

inline int mx_blocks(int64_t n)
{
  const int64_t b = (n + MX_THREADS - 1) / MX_THREADS;
  return (int)(b < MX_MAXBLOCKS ? (b < 1 ? 1 : b) : MX_MAXBLOCKS);
}

// what the kernels read of a handle
struct FillArgs
{
  SpaceArgs s;
  const int32_t* cell_dofs;
  const double *cellJ, *coeff;
  double pi_1;
  ReactArgs rx;
  ShearArgs sx;
  DiffArgs dx;
  const uint8_t* fixed; // nullptr: the raw operator
  const int64_t* sptr;
  const int32_t *srow, *scol;
  int64_t snnz;
  double* values;
};

__global__ void __launch_bounds__(MX_THREADS)
k_matrix_keys(int64_t nkeys, int nd, int64_t ndofs, const int32_t* __restrict__ cell_dofs,
              unsigned long long* __restrict__ keys)
{
  const int nn = nd * nd;
  for (int64_t e = (int64_t)blockIdx.x * MX_THREADS + threadIdx.x; e < nkeys; e += (int64_t)gridDim.x * MX_THREADS)
  {
    const int64_t c = e / nn;
    const int q = (int)(e - c * nn), i = q / nd, j = q - i * nd;
    keys[e] = (unsigned long long)cell_dofs[c * nd + i] * (unsigned long long)ndofs
              + (unsigned long long)cell_dofs[c * nd + j];
  }
}

// one thread per pair e: its row and column; sptr[r] = e for every row r that begins at e (the rows behind the row of
// pair e - 1, empty ones included), and behind the last pair sptr[r] = snnz up to r = ndofs
__global__ void __launch_bounds__(MX_THREADS)
k_matrix_rows(int64_t snnz, int64_t ndofs, const unsigned long long* __restrict__ keys, int64_t* __restrict__ sptr,
              int32_t* __restrict__ srow, int32_t* __restrict__ scol)
{
  for (int64_t e = (int64_t)blockIdx.x * MX_THREADS + threadIdx.x; e < snnz; e += (int64_t)gridDim.x * MX_THREADS)
  {
    const unsigned long long k = keys[e];
    const int64_t row = (int64_t)(k / (unsigned long long)ndofs);
    srow[e] = (int32_t)row;
    scol[e] = (int32_t)(k - (unsigned long long)row * (unsigned long long)ndofs);
    const int64_t prev = e ? (int64_t)(keys[e - 1] / (unsigned long long)ndofs) : -1;
    for (int64_t r = prev + 1; r <= row; ++r)
      sptr[r] = e;
    if (e == snnz - 1)
      for (int64_t r = row + 1; r <= ndofs; ++r)
        sptr[r] = snnz;
  }
}

// indptr [BS ndofs + 1] and indices [BS BS snnz] of the blocked matrix from the scalar pattern
template <int BS>
__global__ void __launch_bounds__(MX_THREADS)
k_matrix_export(int64_t ndofs, int64_t snnz, const int64_t* __restrict__ sptr, const int32_t* __restrict__ srow,
                const int32_t* __restrict__ scol, int64_t* __restrict__ indptr, int32_t* __restrict__ indices)
{
  const int64_t t0 = (int64_t)blockIdx.x * MX_THREADS + threadIdx.x, step = (int64_t)gridDim.x * MX_THREADS;
  if (indptr)
    for (int64_t e = t0; e <= BS * ndofs; e += step)
    {
      if (e == BS * ndofs)
      {
        indptr[e] = BS * BS * snnz;
        continue;
      }
      const int64_t d = e / BS, r = e - d * BS;
      indptr[e] = BS * BS * sptr[d] + r * BS * (sptr[d + 1] - sptr[d]);
    }
  if (indices)
    for (int64_t e = t0; e < snnz; e += step)
    {
      const int64_t d = srow[e], first = sptr[d], len = sptr[d + 1] - first;
#pragma unroll
      for (int r = 0; r < BS; ++r)
#pragma unroll
        for (int s = 0; s < BS; ++s)
          indices[BS * BS * first + r * BS * len + BS * (e - first) + s] = BS * scol[e] + s;
    }
}

template <int BS, int P, bool RX, bool VX>
__global__ void __launch_bounds__(MX_THREADS) k_matrix_fill(const FillArgs a)
{
#pragma clang fp contract(off) // the statement rounds every product and every sum on its own
  constexpr int NP = nd_of(P), NN = NP * NP;
  static_assert(BS == 1 || BS == 2, "Poisson or elasticity");
  const SpaceArgs& sp = a.s;
  const int64_t nshared = (int64_t)sp.nnodes + (int64_t)sp.nfacets * sp.ne;
  for (int64_t e = (int64_t)blockIdx.x * MX_THREADS + threadIdx.x; e < a.snnz; e += (int64_t)gridDim.x * MX_THREADS)
  {
    const int64_t d = a.srow[e];
    const int32_t dc = a.scol[e];
    int64_t beg = 0;
    int cnt = 1;
    int64_t own = 0; // the one entry of an interior DOF
    if (d < nshared)
      slot_range(sp, d, beg, cnt);
    else
    {
      const int64_t q = d - nshared, c = q / sp.ni;
      own = c * NP + 3 + 3 * sp.ne + (q - c * sp.ni);
    }
    double acc[BS][BS];
#pragma unroll
    for (int r = 0; r < BS; ++r)
#pragma unroll
      for (int s = 0; s < BS; ++s)
        acc[r][s] = 0.0;
    bool first = true;
    for (int k = 0; k < cnt; ++k)
    {
      const int64_t flat = d < nshared ? (int64_t)sp.slots[beg + k] : own;
      const int64_t c = flat / NP;
      const int i = (int)(flat - c * NP);
      int j = -1;
      const int32_t* row = a.cell_dofs + c * NP;
#pragma unroll
      for (int jj = 0; jj < NP; ++jj)
        j = (row[jj] == dc) ? jj : j;
      if (j < 0)
        continue; // (this cell of the row's DOF does not hold the column's)
      const double2* Jp = reinterpret_cast<const double2*>(a.cellJ + 4 * c);
      const double2 r0 = Jp[0], r1 = Jp[1]; // J00 J01 | J10 J11
      const double det = r0.x * r1.y - r0.y * r1.x;
      const double adet = fabs(det);
      const double idet = 1.0 / det;
      const int ij = i * NP + j;
      [[maybe_unused]] double wm = 0.0;
      if constexpr (RX)
        wm = (a.rx.cell_c ? a.rx.cell_c[c] : a.rx.c) * adet;
      double v[BS][BS];
      if constexpr (BS == 1)
      {
        const double K00 = r1.y * idet, K01 = -r0.y * idet, K10 = -r1.x * idet, K11 = r0.x * idet;
        double C00, C01, C11;
        if constexpr (VX)
        {
          const double* Dp = a.dx.cell_D + 3 * c;
          const double d00 = Dp[0], d01 = Dp[1], d11 = Dp[2];
          const double T00 = K00 * d00 + K01 * d01, T01 = K00 * d01 + K01 * d11;
          const double T10 = K10 * d00 + K11 * d01, T11 = K10 * d01 + K11 * d11;
          C00 = T00 * K00 + T01 * K01;
          C01 = T00 * K10 + T01 * K11;
          C11 = T10 * K10 + T11 * K11;
        }
        else
        {
          C00 = K00 * K00 + K01 * K01;
          C01 = K00 * K10 + K01 * K11;
          C11 = K10 * K10 + K11 * K11;
        }
        const double w = (a.coeff ? a.coeff[c] : 1.0) * adet;
        const double* ST = eqlb_tables::Stiff<P>::ST;
        double x = w * ((C00 * ST[ij] + C01 * ST[NN + ij]) + C11 * ST[2 * NN + ij]);
        if constexpr (RX)
          x = x + wm * eqlb_tables::Mass<P>::MS[ij];
        v[0][0] = x;
      }
      else
      {
        const double K[2][2] = {{r1.y * idet, -r0.y * idet}, {-r1.x * idet, r0.x * idet}}; // K[X][d]
        const double* ST = eqlb_tables::Stiff<P>::ST;
        const double* CR = eqlb_tables::Cross<P>::CR;
        const double g[4] = {ST[ij], CR[ij], CR[j * NP + i], ST[2 * NN + ij]}; // g_00, g_01, g_10, g_11
        double Dd[2][2];
#pragma unroll
        for (int aa = 0; aa < 2; ++aa)
#pragma unroll
          for (int bb = 0; bb < 2; ++bb)
            Dd[aa][bb] = ((K[0][aa] * K[0][bb]) * g[0] + (K[0][aa] * K[1][bb]) * g[1])
                         + ((K[1][aa] * K[0][bb]) * g[2] + (K[1][aa] * K[1][bb]) * g[3]);
        const double pi = a.coeff ? a.coeff[c] : a.pi_1;
        [[maybe_unused]] double mu = 1.0;
        if constexpr (VX)
          mu = a.sx.cell_mu ? a.sx.cell_mu[c] : a.sx.mu;
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
          for (int s = 0; s < 2; ++s)
          {
            double x = r == s ? adet * (((Dd[0][0] + Dd[1][1]) + Dd[r][r]) + pi * Dd[r][r])
                              : adet * (Dd[s][r] + pi * Dd[r][s]);
            if constexpr (VX) // one product on top of the value formed without the term
              x = mu * x;
            if constexpr (RX)
              if (r == s) // the reaction term is not scaled, and couples no components
                x = x + wm * eqlb_tables::Mass<P>::MS[ij];
            v[r][s] = x;
          }
      }
#pragma unroll
      for (int r = 0; r < BS; ++r)
#pragma unroll
        for (int s = 0; s < BS; ++s)
          acc[r][s] = first ? v[r][s] : acc[r][s] + v[r][s];
      first = false;
    }
    const int64_t p0 = a.sptr[d], len = a.sptr[d + 1] - p0;
#pragma unroll
    for (int r = 0; r < BS; ++r)
#pragma unroll
      for (int s = 0; s < BS; ++s)
      {
        double x = acc[r][s];
        if (a.fixed && (a.fixed[BS * d + r] || a.fixed[BS * (int64_t)dc + s]))
          x = (d == dc && r == s) ? 1.0 : 0.0; // P A P + (I - P)
        a.values[BS * BS * p0 + r * BS * len + BS * (e - p0) + s] = x;
      }
  }
}

// The facet term of a handle on top of the filled values: one thread per DOF d that lies in a listed facet walks the
// facets of the DOF in ascending id (the table of the sum pass) and adds to the entries of every DOF d_j of the facet,
// each by one addition - the cell sums first, then the facets ascending, as the statement has it; the diagonal entry
// gets the bits of the handle's diagonal.  An eliminated entry keeps its 0.0 or 1.0.
//   BS = 1  the Robin term (include/eqlb.h: eqlb_primal_set_robin): w_f FacetMass[i][j] to the entry (d, d_j).  The
//           pattern holds every such pair (both rows lie in the facet's cell)
//   BS = 2  the spring term (eqlb_elasticity_set_springs): Kw[r][s] FacetMass[i][j] to the entry (2 d + r, 2 d_j + s).
//           The pattern is the scalar one and every pair of DOFs of a cell carries its full 2 x 2 block, so every such
//           entry exists: row 2 d + r starts at 4 sptr[d] + 2 r len(d), and pair k of the row holds the columns at 2 k + s
struct FacetFillArgs
{
  int32_t m, n1;
  const int32_t *rows, *off, *ent, *dofs;
  const double *w, *fm; // w: [nlist] (BS = 1) or [nlist][3] (BS = 2), FacetTermArgs
  const uint8_t* fixed; // [BS ndofs]; nullptr: the raw operator
  const int64_t* sptr;
  const int32_t* scol;
  double* values;
};

template <int BS>
__global__ void __launch_bounds__(MX_THREADS) k_matrix_facet(const FacetFillArgs a)
{
#pragma clang fp contract(off)
  for (int32_t mi = blockIdx.x * MX_THREADS + threadIdx.x; mi < a.m; mi += gridDim.x * MX_THREADS)
  {
    const int64_t d = a.rows[mi];
    const int64_t p0 = a.sptr[d], p1 = a.sptr[d + 1], len = p1 - p0;
    for (int q = a.off[mi]; q < a.off[mi + 1]; ++q)
    {
      const int32_t en = a.ent[q];
      const int i = en & 7;
      const int64_t li = en >> 3;
      const int32_t* dd = a.dofs + li * FACET_ROW;
      const double* w = a.w + (BS == 1 ? 1 : 3) * li;
      for (int j = 0; j < a.n1; ++j)
      {
        const int32_t dc = dd[j];
        if constexpr (BS == 1)
          if (a.fixed && (a.fixed[d] || a.fixed[dc]))
            continue;
        int64_t lo = p0, hi = p1;
        while (lo < hi)
        {
          const int64_t mid = (lo + hi) >> 1;
          if (a.scol[mid] < dc)
            lo = mid + 1;
          else
            hi = mid;
        }
        if (!(lo < p1 && a.scol[lo] == dc))
          continue;
        const double f = a.fm[i * a.n1 + j];
        if constexpr (BS == 1)
          a.values[lo] = a.values[lo] + w[0] * f;
        else
          for (int r = 0; r < 2; ++r)
            for (int s = 0; s < 2; ++s)
            {
              if (a.fixed && (a.fixed[2 * d + r] || a.fixed[2 * (int64_t)dc + s]))
                continue;
              const int64_t pos = 4 * p0 + r * 2 * len + 2 * (lo - p0) + s;
              a.values[pos] = a.values[pos] + w[r + s] * f;
            }
      }
    }
  }
}

// y[row] = the sum over the positions of the row in ascending order, the first product starts it.  One row per thread;
// a bundle of G consecutive rows (the rows of G neighbouring lanes) one of which has CSR_GROUP_MIN entries or more is
// summed by the G lanes together, row after row: the lanes read G consecutive entries of the row at once and form the
// G products, which every lane then adds in their order from its neighbours' registers - the same products, the same
// order and so the same bits as the one-thread sum, with the loads of a long row side by side instead of a row apart.
// The choice is made per bundle on the device (a call in device memory space does not know nnz on the host).
template <int G>
__global__ void __launch_bounds__(MX_THREADS)
k_csr_apply(int64_t n, const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
            const double* __restrict__ values, const double* __restrict__ x, double* __restrict__ y, int64_t group_min)
{
#pragma clang fp contract(off)
  static_assert(G >= 2 && G <= 64 && (G & (G - 1)) == 0 && MX_THREADS % G == 0, "lanes of a bundle");
  const int lane = threadIdx.x & (G - 1);
  // (the stride is a multiple of G, so the lanes of a bundle stay together and leave the loop together)
  for (int64_t base = (int64_t)blockIdx.x * MX_THREADS + threadIdx.x - lane; base < n;
       base += (int64_t)gridDim.x * MX_THREADS)
  {
    const int64_t row = base + lane;
    const int64_t b = row < n ? indptr[row] : 0, e = row < n ? indptr[row + 1] : 0;
    int64_t longest = e - b;
#pragma unroll
    for (int m = G / 2; m > 0; m >>= 1)
    {
      const int64_t other = __shfl_xor(longest, m, G);
      longest = other > longest ? other : longest;
    }
    double mine = 0.0;
    if (longest < group_min)
    {
      if (b < e)
        mine = values[b] * x[indices[b]];
      for (int64_t k = b + 1; k < e; ++k)
        mine = mine + values[k] * x[indices[k]];
    }
    else
    {
      for (int r = 0; r < G; ++r)
      {
        const int64_t rb = __shfl(b, r, G), re = __shfl(e, r, G);
        double s = 0.0;
        for (int64_t k0 = rb; k0 < re; k0 += G)
        {
          const int64_t k = k0 + lane;
          const double prod = k < re ? values[k] * x[indices[k]] : 0.0;
          const int cnt = re - k0 < G ? (int)(re - k0) : G;
#pragma unroll
          for (int j = 0; j < G; ++j)
          {
            const double t = __shfl(prod, j, G);
            if (j < cnt)
              s = (k0 == rb && j == 0) ? t : s + t;
          }
        }
        mine = lane == r ? s : mine;
      }
    }
    if (row < n)
      y[row] = mine;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------
template <int BS, int P>
hipError_t launch_fill_p(const MatrixView& v, const FillArgs& a, hipStream_t stream)
{
  const dim3 grid(mx_blocks(a.snnz)), block(MX_THREADS);
  const bool vx = BS == 1 ? v.has_diff : v.has_shear;
  if (v.has_react && vx)
    hipLaunchKernelGGL((k_matrix_fill<BS, P, true, true>), grid, block, 0, stream, a);
  else if (v.has_react)
    hipLaunchKernelGGL((k_matrix_fill<BS, P, true, false>), grid, block, 0, stream, a);
  else if (vx)
    hipLaunchKernelGGL((k_matrix_fill<BS, P, false, true>), grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL((k_matrix_fill<BS, P, false, false>), grid, block, 0, stream, a);
  return hipGetLastError();
}

template <int BS>
hipError_t launch_fill(const MatrixView& v, bool eliminate, double* values, hipStream_t stream)
{
  const MatrixPattern& pt = *v.pattern;
  FillArgs a{};
  a.s = v.s;
  a.cell_dofs = v.cell_dofs;
  a.cellJ = v.cellJ;
  a.coeff = v.coeff;
  a.pi_1 = v.pi_1;
  a.rx = v.rx;
  a.sx = v.sx;
  a.dx = v.dx;
  a.fixed = eliminate ? v.fixed : nullptr;
  a.sptr = pt.sptr;
  a.srow = pt.srow;
  a.scol = pt.scol;
  a.snnz = pt.snnz;
  a.values = values;
  switch (v.p)
  {
  case 1:
    return launch_fill_p<BS, 1>(v, a, stream);
  case 2:
    return launch_fill_p<BS, 2>(v, a, stream);
  case 3:
    return launch_fill_p<BS, 3>(v, a, stream);
  default:
    return launch_fill_p<BS, 4>(v, a, stream);
  }
}

// the pattern of the handle behind v, built on `stream` at the first call (which waits for the count)
int matrix_pattern(const char* who, MatrixView& v, int64_t* nnz, hipStream_t stream)
{
  if (!nnz)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  MatrixPattern& pt = *v.pattern;
  const int64_t bb = (int64_t)v.bs * v.bs;
  if (pt.built)
  {
    *nnz = bb * pt.snnz;
    return EQLB_OK;
  }
  const MatrixPlan plan = matrix_plan(v.bs, v.s.nd, v.s.ncells, v.s.ndofs);
  if (!plan.ok)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: %lld rows or %lld keys are more than the index types hold", who,
                (long long)plan.rows, (long long)plan.nkeys);
  const size_t nkeys = (size_t)plan.nkeys;
  DevCarve pool;
  const auto p_in = pool.piece<unsigned long long>(nkeys), p_out = pool.piece<unsigned long long>(nkeys);
  const auto p_count = pool.piece<unsigned long long>(1);
  if (pool.alloc() != hipSuccess)
    return fail(EQLB_ERR_NO_MEMORY, "%s: device allocation of %zu bytes for the keys failed", who, pool.bytes());
  unsigned long long *keys_in = p_in, *keys_out = p_out, *count = p_count;
  size_t t_sort = 0, t_uniq = 0;
  HIP_TRY(rocprim::radix_sort_keys(nullptr, t_sort, keys_in, keys_out, nkeys, 0u, plan.key_bits, stream));
  HIP_TRY(rocprim::unique(nullptr, t_uniq, keys_out, keys_in, count, nkeys, rocprim::equal_to<unsigned long long>(),
                          stream));
  const size_t tmp_bytes = t_sort > t_uniq ? t_sort : t_uniq;
  DevBuf<char> tmp;
  if (tmp.alloc_raw(tmp_bytes) != hipSuccess)
    return fail(EQLB_ERR_NO_MEMORY, "%s: device allocation of %zu bytes failed", who, tmp_bytes);
  hipLaunchKernelGGL(k_matrix_keys, dim3(mx_blocks(plan.nkeys)), dim3(MX_THREADS), 0, stream, plan.nkeys, v.s.nd, v.s.ndofs,
                     v.cell_dofs, keys_in);
  HIP_TRY(hipGetLastError());
  {
    size_t tb = tmp_bytes;
    HIP_TRY(rocprim::radix_sort_keys(tmp.get(), tb, keys_in, keys_out, nkeys, 0u, plan.key_bits, stream));
  }
  {
    size_t tb = tmp_bytes;
    HIP_TRY(rocprim::unique(tmp.get(), tb, keys_out, keys_in, count, nkeys, rocprim::equal_to<unsigned long long>(),
                            stream));
  }
  unsigned long long found = 0;
  HIP_TRY(hipMemcpyAsync(&found, count, sizeof(found), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  if (found < 1 || found > nkeys || !matrix_count_fits(v.bs, (int64_t)found))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: %llu entries per block are more than the index types hold", who, found);
  const int64_t snnz = (int64_t)found;
  MatrixPattern fresh;
  if (fresh.sptr.alloc_raw((size_t)v.s.ndofs + 1) != hipSuccess || fresh.srow.alloc_raw((size_t)snnz) != hipSuccess
      || fresh.scol.alloc_raw((size_t)snnz) != hipSuccess)
    return fail(EQLB_ERR_NO_MEMORY, "%s: device allocation of the pattern (%lld pairs) failed", who, (long long)snnz);
  hipLaunchKernelGGL(k_matrix_rows, dim3(mx_blocks(snnz)), dim3(MX_THREADS), 0, stream, snnz, v.s.ndofs, keys_in,
                     fresh.sptr.get(), fresh.srow.get(), fresh.scol.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(stream)); // (the keys end with this call)
  fresh.snnz = snnz;
  fresh.built = true;
  fresh.peak_bytes = pool.bytes() + tmp_bytes + matrix_kept_bytes(v.s.ndofs, snnz);
  if (getenv("EQLB_PROFILE_SETUP")) // (the switch of SetupTimer)
    fprintf(stderr, "[eqlb setup] %s: %lld keys, %lld pairs, peak work space %zu bytes (kept %zu)\n", who,
            (long long)plan.nkeys, (long long)snnz, fresh.peak_bytes, matrix_kept_bytes(v.s.ndofs, snnz));
  pt = std::move(fresh);
  *nnz = bb * snnz;
  return EQLB_OK;
}

int need_pattern(const char* who, const MatrixView& v)
{
  if (!v.pattern->built)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: no pattern (eqlb_%s_matrix_pattern first)", who,
                v.bs == 1 ? "primal" : "elasticity");
  return EQLB_OK;
}

int matrix_export(const char* who, const MatrixView& v, int64_t* indptr, int32_t* indices, int32_t memspace,
                  void* stream_)
{
  if (!indptr || !indices)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  EQLB_TRY(check_memspace(who, memspace));
  EQLB_TRY(need_pattern(who, v));
  const MatrixPattern& pt = *v.pattern;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool host = memspace == EQLB_MEM_HOST;
  const size_t n = (size_t)v.bs * v.s.ndofs, nnz = (size_t)v.bs * v.bs * pt.snnz;
  HostCall s;
  const auto d_p = s.out(host ? indptr : nullptr, n + 1);
  const auto d_i = s.out(host ? indices : nullptr, nnz);
  if (host)
    HIP_TRY(s.upload(stream));
  int64_t* pp = host ? d_p.get() : indptr;
  int32_t* pi = host ? d_i.get() : indices;
  const int64_t most = pt.snnz > (int64_t)n + 1 ? pt.snnz : (int64_t)n + 1;
  const dim3 grid(mx_blocks(most)), block(MX_THREADS);
  if (v.bs == 1)
    hipLaunchKernelGGL(k_matrix_export<1>, grid, block, 0, stream, v.s.ndofs, pt.snnz, pt.sptr.get(), pt.srow.get(),
                       pt.scol.get(), pp, pi);
  else
    hipLaunchKernelGGL(k_matrix_export<2>, grid, block, 0, stream, v.s.ndofs, pt.snnz, pt.sptr.get(), pt.srow.get(),
                       pt.scol.get(), pp, pi);
  s.note(hipGetLastError());
  HIP_TRY(s.finish(stream));
  return EQLB_OK;
}

int matrix_values(const char* who, const MatrixView& v, int32_t eliminate, double* values, int64_t capacity,
                  int32_t memspace, void* stream_)
{
  if (!values)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  if (eliminate != 0 && eliminate != 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: eliminate = %d (0 or 1)", who, (int)eliminate);
  EQLB_TRY(check_memspace(who, memspace));
  EQLB_TRY(need_pattern(who, v));
  const int64_t nnz = (int64_t)v.bs * v.bs * v.pattern->snnz;
  if (capacity < nnz)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: capacity = %lld is less than nnz = %lld", who, (long long)capacity,
                (long long)nnz);
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool host = memspace == EQLB_MEM_HOST;
  HostCall s;
  const auto d_v = s.out(host ? values : nullptr, (size_t)nnz);
  if (host)
    HIP_TRY(s.upload(stream));
  double* pv = host ? d_v.get() : values;
  s.note(v.bs == 1 ? launch_fill<1>(v, eliminate != 0, pv, stream) : launch_fill<2>(v, eliminate != 0, pv, stream));
  if (v.has_facet && v.facet_m > 0)
  {
    const FacetTermArgs& x = v.facet;
    const FacetFillArgs a{v.facet_m, x.n1, x.rows, x.off, x.ent, x.dofs, x.w, x.fm, eliminate ? v.fixed : nullptr,
                          v.pattern->sptr.get(), v.pattern->scol.get(), pv};
    const dim3 grid(mx_blocks(v.facet_m)), block(MX_THREADS);
    if (v.bs == 1)
      hipLaunchKernelGGL(k_matrix_facet<1>, grid, block, 0, stream, a);
    else
      hipLaunchKernelGGL(k_matrix_facet<2>, grid, block, 0, stream, a);
    s.note(hipGetLastError());
  }
  HIP_TRY(s.finish(stream));
  return EQLB_OK;
}
} // namespace
} // namespace eqlb

extern "C" {

int eqlb_primal_matrix_pattern(eqlb_primal_t* h, int64_t* nnz, void* stream)
try
{
  using namespace eqlb;
  EQLB_TRY(check_handle("eqlb_primal_matrix_pattern", h));
  MatrixView v;
  primal_matrix_view(h, v);
  return matrix_pattern("eqlb_primal_matrix_pattern", v, nnz, reinterpret_cast<hipStream_t>(stream));
}
EQLB_CATCH_ALL

int eqlb_primal_matrix_export(eqlb_primal_t* h, int64_t* indptr, int32_t* indices, int32_t memspace, void* stream)
try
{
  using namespace eqlb;
  EQLB_TRY(check_handle("eqlb_primal_matrix_export", h));
  MatrixView v;
  primal_matrix_view(h, v);
  return matrix_export("eqlb_primal_matrix_export", v, indptr, indices, memspace, stream);
}
EQLB_CATCH_ALL

int eqlb_primal_matrix_values(eqlb_primal_t* h, int32_t eliminate, double* values, int64_t capacity, int32_t memspace,
                              void* stream)
try
{
  using namespace eqlb;
  EQLB_TRY(check_handle("eqlb_primal_matrix_values", h));
  MatrixView v;
  primal_matrix_view(h, v);
  return matrix_values("eqlb_primal_matrix_values", v, eliminate, values, capacity, memspace, stream);
}
EQLB_CATCH_ALL

void eqlb_primal_matrix_release(eqlb_primal_t* h)
{
  if (!h)
    return;
  eqlb::MatrixView v;
  eqlb::primal_matrix_view(h, v);
  *v.pattern = eqlb::MatrixPattern{};
}

int eqlb_elasticity_matrix_pattern(eqlb_elasticity_t* h, int64_t* nnz, void* stream)
try
{
  using namespace eqlb;
  EQLB_TRY(check_handle("eqlb_elasticity_matrix_pattern", h));
  MatrixView v;
  elasticity_matrix_view(h, v);
  return matrix_pattern("eqlb_elasticity_matrix_pattern", v, nnz, reinterpret_cast<hipStream_t>(stream));
}
EQLB_CATCH_ALL

int eqlb_elasticity_matrix_export(eqlb_elasticity_t* h, int64_t* indptr, int32_t* indices, int32_t memspace,
                                  void* stream)
try
{
  using namespace eqlb;
  EQLB_TRY(check_handle("eqlb_elasticity_matrix_export", h));
  MatrixView v;
  elasticity_matrix_view(h, v);
  return matrix_export("eqlb_elasticity_matrix_export", v, indptr, indices, memspace, stream);
}
EQLB_CATCH_ALL

int eqlb_elasticity_matrix_values(eqlb_elasticity_t* h, int32_t eliminate, double* values, int64_t capacity,
                                  int32_t memspace, void* stream)
try
{
  using namespace eqlb;
  EQLB_TRY(check_handle("eqlb_elasticity_matrix_values", h));
  MatrixView v;
  elasticity_matrix_view(h, v);
  return matrix_values("eqlb_elasticity_matrix_values", v, eliminate, values, capacity, memspace, stream);
}
EQLB_CATCH_ALL

void eqlb_elasticity_matrix_release(eqlb_elasticity_t* h)
{
  if (!h)
    return;
  eqlb::MatrixView v;
  eqlb::elasticity_matrix_view(h, v);
  *v.pattern = eqlb::MatrixPattern{};
}

int eqlb_csr_apply(int64_t n, const int64_t* indptr, const int32_t* indices, const double* values, const double* x,
                   double* y, int32_t memspace, void* stream_)
try
{
  using namespace eqlb;
  const char* who = "eqlb_csr_apply";
  if (!indptr || !indices || !values || !x || !y)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  if (n < 0 || n > INT32_MAX)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: n = %lld outside 0 ... 2^31 - 1, the range of the column indices", who,
                (long long)n);
  EQLB_TRY(check_memspace(who, memspace));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool host = memspace == EQLB_MEM_HOST;
  if (n == 0)
    return EQLB_OK;
  HostCall s;
  size_t nnz = 0;
  if (host)
  {
    // a host matrix is checked before anything is launched: offsets that do not fall, columns inside the matrix
    if (indptr[0] != 0)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: indptr[0] = %lld (0 expected)", who, (long long)indptr[0]);
    for (int64_t r = 0; r < n; ++r)
      if (indptr[r + 1] < indptr[r])
        return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: indptr[%lld] = %lld falls below indptr[%lld] = %lld", who,
                    (long long)(r + 1), (long long)indptr[r + 1], (long long)r, (long long)indptr[r]);
    nnz = (size_t)indptr[n];
    for (size_t k = 0; k < nnz; ++k)
      if (indices[k] < 0 || indices[k] >= n)
        return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: indices[%lld] = %d is no column of the matrix (%lld columns)", who,
                    (long long)k, (int)indices[k], (long long)n);
  }
  const auto d_p = s.in(host ? indptr : nullptr, (size_t)n + 1);
  const auto d_i = s.in(host ? indices : nullptr, nnz);
  const auto d_v = s.in(host ? values : nullptr, nnz);
  const auto d_x = s.in(host ? x : nullptr, (size_t)n);
  const auto d_y = s.out(host ? y : nullptr, (size_t)n);
  if (host)
    HIP_TRY(s.upload(stream));
  hipLaunchKernelGGL(k_csr_apply<CSR_GROUP>, dim3(stream_blocks(n)), dim3(MX_THREADS), 0, stream, n,
                     host ? d_p.get() : indptr, host ? d_i.get() : indices, host ? d_v.get() : values,
                     host ? d_x.get() : x, host ? d_y.get() : y, (int64_t)CSR_GROUP_MIN);
  s.note(hipGetLastError());
  HIP_TRY(s.finish(stream));
  return EQLB_OK;
}
EQLB_CATCH_ALL

} // extern "C"
