// The exact solve on the coarsest level of a hierarchy ON THE DEVICE: eqlb_hierarchy_set_coarse of include/eqlb.h behind
// eqlb_multilevel.hip.  The rule is stated as numpy in dolfinx_eqlb_amd/lsolver/multilevel.py (Hierarchy(...,
// coarse=True): coarse_matrix, coarse_factor, coarse_solve); factor and application reproduce it bit for bit.
//
// Set-up (coarse_setup), once per eqlb_hierarchy_set_coarse(h, 1):
//  rows   the free rows of level 0 from its mask, compacted on the host (the call waits anyway), at most COARSE_MAX_ROWS
//  A_0    column by column from the product launches of the level-0 handle on unit vectors (k_coarse_units, the
//         handle's own launches, k_coarse_pick), MANY_R columns at a time on a Poisson handle: the bits of apply
//  factor the right-looking LDL^T of the statement, blocked by COARSE_BLOCK columns:
//         k_coarse_panel    the block of columns k0 ... k0 + nb - 1 on the rows i >= k0, one thread per row with the
//                           entries of its row in registers; every workgroup first eliminates the diagonal block in LDS
//                           (the values c_j of the rows of the block that the rows below need).  Writes the
//                           multipliers l into the panel [n][COARSE_BLOCK], the pivots into d
//         k_coarse_trail<0> a_ij -= l_ik c_jk on the trailing lower triangle in tiles of COARSE_TILE x COARSE_TILE from LDS
//         k_coarse_wpanel   the rows of the block of W = L^-1: one thread per column
//         k_coarse_trail<1> w_ij -= l_ik w_kj on the rows below the block, the same tiles
//         A thread that owns an entry applies the k of the block ascending, every product and every difference rounded
//         on its own (contraction off): the bits of the rank-1 statement.  fp64 matrix instructions fuse the rounding
//         and are not used; this is vector ALU work, about n^3 / 3 multiply-subtract pairs per factor
//  k_coarse_transpose   W^T into the memory of A_0, so that both passes of an application read coalesced
// A pivot that is not > 0 (or NaN) leaves 1 + its index in the status word; nothing that is computed behind it is used.
//
// Application (coarse_apply), two launches with the column slots and stop flags of the k_ml_* kernels:
//  k_coarse_forward   y_i = (sum_{k <= i} w_ik r[rows[k]]) / d_i, one thread per row, k ascending, from W^T
//  k_coarse_backward  z[rows[j]] = sum_{i >= j} w_ij y_i, one thread per column, i ascending, from W; 0 on the fixed rows
// W is read once for up to MANY_R columns.
#include "eqlb_device_common.h"
#include "eqlb_coarse.h"
#include "eqlb_tuning.h"

#include <algorithm>
#include <vector>

namespace eqlb
{
namespace
{
constexpr int COARSE_MAX_ROWS = EQLB_COARSE_MAX_ROWS;
constexpr int CB = EQLB_COARSE_BLOCK; // columns of a block step
constexpr int CT = EQLB_COARSE_TILE;  // rows and columns of a tile of the trailing updates; threads of the row kernels
constexpr int TRAIL_THREADS = 256;    // 16 x 16 threads, (CT / 16)^2 entries each
constexpr int CM = CT / 16;
constexpr int UNIT_THREADS = 256;
static_assert(CB >= 2 && CB <= 32 && CT % 16 == 0 && CT >= CB && CT <= 64, "EQLB_COARSE_BLOCK, EQLB_COARSE_TILE");
static_assert((CT * CB) % TRAIL_THREADS == 0, "the tiles are loaded in whole rounds of the workgroup");

// ---- A_0 -----------------------------------------------------------------------------------------------------------
// the unit vectors of the free rows j0 ... j0 + R - 1 as the R columns of the direction of the level-0 handle
__global__ void __launch_bounds__(UNIT_THREADS)
k_coarse_units(int64_t n0, int R, int32_t n, int32_t j0, const int32_t* __restrict__ rows, double* __restrict__ dir)
{
  for (int64_t e = (int64_t)blockIdx.x * UNIT_THREADS + threadIdx.x; e < n0; e += (int64_t)gridDim.x * UNIT_THREADS)
    for (int c = 0; c < R; ++c)
      dir[c * n0 + e] = (j0 + c < n && rows[j0 + c] == e) ? 1.0 : 0.0;
}

// columns j0 ... j0 + R - 1 of A_0 from the products q [R][n0]
__global__ void __launch_bounds__(UNIT_THREADS)
k_coarse_pick(int64_t n0, int R, int32_t n, int32_t j0, const int32_t* __restrict__ rows, const double* __restrict__ q,
              double* __restrict__ A)
{
  const int64_t i = (int64_t)blockIdx.x * UNIT_THREADS + threadIdx.x;
  if (i >= n)
    return;
  const int64_t row = rows[i];
  if (row < 0 || row >= n0)
    return;
  for (int c = 0; c < R; ++c)
    if (j0 + c < n)
      A[i * n + j0 + c] = q[c * n0 + row];
}

__global__ void __launch_bounds__(UNIT_THREADS) k_coarse_unit_diagonal(int32_t n, double* __restrict__ W)
{
  const int64_t i = (int64_t)blockIdx.x * UNIT_THREADS + threadIdx.x;
  if (i < n)
    W[i * n + i] = 1.0;
}

// ---- the factor ----------------------------------------------------------------------------------------------------
// The columns k0 ... k0 + nb - 1 (nb <= CB) on the rows i >= k0, one thread per row.  For row i and the steps k of the
// block with k0 + k < i: l = a_ik / d_k, a_ij -= l c_jk for the columns j of the block with k < j and k0 + j <= i.  c_jk
// (row k0 + j at step k) comes from the diagonal block, which every workgroup eliminates in LDS first - the same
// operations, so the same bits everywhere.  Workgroup 0 writes the pivots and looks at their sign.
__global__ void __launch_bounds__(CT)
k_coarse_panel(int32_t n, int32_t k0, int32_t nb, double* __restrict__ A, double* __restrict__ panel,
               double* __restrict__ d, int32_t* __restrict__ status)
{
#pragma clang fp contract(off)
  __shared__ double D[CB][CB + 1];
  const int t = threadIdx.x;
  if (t < CB)
    for (int j = 0; j < CB; ++j)
      D[t][j] = (t < nb && j <= t) ? A[(int64_t)(k0 + t) * n + k0 + j] : 0.0;
  for (int k = 0; k < nb; ++k)
  {
    __syncthreads(); // (column k is complete: it was written in the steps before k)
    if (t > k && t < nb)
    {
      const double l = D[t][k] / D[k][k];
      for (int j = k + 1; j <= t; ++j)
        D[t][j] = D[t][j] - l * D[j][k];
    }
  }
  __syncthreads();
  if (blockIdx.x == 0)
  {
    if (t < nb)
      d[k0 + t] = D[t][t];
    if (t == 0 && status[0] == 0)
      for (int k = 0; k < nb; ++k)
        if (!(D[k][k] > 0.0))
        {
          status[0] = k0 + k + 1;
          break;
        }
  }
  const int64_t i = (int64_t)k0 + (int64_t)blockIdx.x * CT + t;
  if (i >= n)
    return;
  const int reach = (int)(i - k0 < nb ? i - k0 : nb - 1); // the last column of the block in the lower triangle of row i
  double a[CB];
#pragma unroll
  for (int j = 0; j < CB; ++j)
    a[j] = j <= reach ? A[i * n + k0 + j] : 0.0;
#pragma unroll
  for (int k = 0; k < CB; ++k)
  {
    double l = 0.0;
    if (k < nb && k0 + k < i)
    {
      l = a[k] / D[k][k];
#pragma unroll
      for (int j = k + 1; j < CB; ++j)
        if (j <= reach)
          a[j] = a[j] - l * D[j][k];
    }
    panel[i * CB + k] = l;
  }
  // The rows of the diagonal block are not written back: the other workgroups may still be reading them, and nothing
  // reads these entries of A again (the later steps take c_jk from the rows below the block only).
  if (i < (int64_t)k0 + nb)
    return;
#pragma unroll
  for (int j = 0; j < CB; ++j)
    if (j <= reach)
      A[i * n + k0 + j] = a[j];
}

// The update of the block k0 ... k0 + CB - 1 on what lies below it, in tiles of CT x CT; s = k0 + CB < n.
//  IS_W = 0  x = A, rows and columns s ... n - 1, the lower triangle (i >= j): a_ij -= l_ik c_jk, c_jk = A[j][k0 + k]
//  IS_W = 1  x = W, rows s ... n - 1, columns 0 ... s - 1: w_ij -= l_ik w_kj for k0 + k >= j, w_kj = W[k0 + k][j]
// Every entry takes the k of the block ascending.
template <int IS_W>
__global__ void __launch_bounds__(TRAIL_THREADS)
k_coarse_trail(int32_t n, int32_t k0, double* __restrict__ X, const double* __restrict__ panel)
{
#pragma clang fp contract(off)
  __shared__ double Ls[CT][CB + 1];
  __shared__ double Bs[CB][CT + 1];
  const int32_t s = k0 + CB;
  if (!IS_W && blockIdx.x > blockIdx.y)
    return; // (a tile above the diagonal)
  const int t = threadIdx.x;
  const int64_t i0 = (int64_t)s + (int64_t)blockIdx.y * CT;
  const int64_t j0 = (IS_W ? 0 : (int64_t)s) + (int64_t)blockIdx.x * CT;
  const int64_t jend = IS_W ? s : n; // columns of x this launch works on end here
  for (int e = t; e < CT * CB; e += TRAIL_THREADS)
  {
    const int r = e / CB, k = e % CB;
    Ls[r][k] = i0 + r < n ? panel[(i0 + r) * CB + k] : 0.0;
    if (IS_W)
    {
      const int kk = e / CT, jj = e % CT;
      Bs[kk][jj] = j0 + jj < jend ? X[(int64_t)(k0 + kk) * n + j0 + jj] : 0.0;
    }
    else
      Bs[k][r] = j0 + r < jend ? X[(j0 + r) * n + k0 + k] : 0.0;
  }
  __syncthreads();
  const int ty = t / 16, tx = t % 16;
  double x[CM][CM];
  bool mine[CM][CM];
#pragma unroll
  for (int a = 0; a < CM; ++a)
#pragma unroll
    for (int b = 0; b < CM; ++b)
    {
      const int64_t i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
      mine[a][b] = i < n && j < jend && (IS_W || i >= j);
      x[a][b] = mine[a][b] ? X[i * n + j] : 0.0;
    }
#pragma unroll 2 // (unrolled completely, the operand loads of all k are hoisted and the registers spill)
  for (int k = 0; k < CB; ++k)
  {
    double la[CM], bv[CM];
#pragma unroll
    for (int a = 0; a < CM; ++a)
      la[a] = Ls[ty + 16 * a][k];
#pragma unroll
    for (int b = 0; b < CM; ++b)
      bv[b] = Bs[k][tx + 16 * b];
#pragma unroll
    for (int a = 0; a < CM; ++a)
#pragma unroll
      for (int b = 0; b < CM; ++b)
      {
        const bool takes = !IS_W || (int64_t)k0 + k >= j0 + tx + 16 * b;
        if (takes)
          x[a][b] = x[a][b] - la[a] * bv[b];
      }
  }
#pragma unroll
  for (int a = 0; a < CM; ++a)
#pragma unroll
    for (int b = 0; b < CM; ++b)
      if (mine[a][b])
        X[(i0 + ty + 16 * a) * n + j0 + tx + 16 * b] = x[a][b];
}

// The rows k0 ... k0 + nb - 1 of W, one thread per column j < k0 + nb: w_rj -= l_rk w_kj for the rows r > k of the block
// and k0 + k >= j, k ascending.  The multipliers of the block's own rows come from the panel.
__global__ void __launch_bounds__(CT)
k_coarse_wpanel(int32_t n, int32_t k0, int32_t nb, double* __restrict__ W, const double* __restrict__ panel)
{
#pragma clang fp contract(off)
  __shared__ double Ld[CB][CB + 1];
  const int t = threadIdx.x;
  for (int e = t; e < CB * CB; e += CT)
  {
    const int r = e / CB, k = e % CB;
    Ld[r][k] = (r < nb && k < r) ? panel[(int64_t)(k0 + r) * CB + k] : 0.0;
  }
  __syncthreads();
  const int64_t j = (int64_t)blockIdx.x * CT + t;
  if (j >= (int64_t)k0 + nb)
    return;
  double w[CB];
#pragma unroll
  for (int r = 0; r < CB; ++r)
    w[r] = r < nb ? W[(int64_t)(k0 + r) * n + j] : 0.0;
#pragma unroll
  for (int k = 0; k < CB - 1; ++k)
    if (k < nb && (int64_t)k0 + k >= j)
    {
#pragma unroll
      for (int r = k + 1; r < CB; ++r)
        if (r < nb)
          w[r] = w[r] - Ld[r][k] * w[k];
    }
#pragma unroll
  for (int r = 1; r < CB; ++r)
    if (r < nb)
      W[(int64_t)(k0 + r) * n + j] = w[r];
}

// Wt = W^T in tiles of CB x CB through LDS
__global__ void __launch_bounds__(UNIT_THREADS)
k_coarse_transpose(int32_t n, const double* __restrict__ W, double* __restrict__ Wt)
{
  __shared__ double T[CB][CB + 1];
  const int64_t i0 = (int64_t)blockIdx.y * CB, j0 = (int64_t)blockIdx.x * CB;
  for (int e = threadIdx.x; e < CB * CB; e += UNIT_THREADS)
  {
    const int r = e / CB, c = e % CB;
    T[r][c] = (i0 + r < n && j0 + c < n) ? W[(i0 + r) * n + j0 + c] : 0.0;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < CB * CB; e += UNIT_THREADS)
  {
    const int r = e / CB, c = e % CB; // entry (j0 + r, i0 + c) of the transpose
    if (j0 + r < n && i0 + c < n)
      Wt[(j0 + r) * n + i0 + c] = T[c][r];
  }
}

// ---- the application -----------------------------------------------------------------------------------------------
// Both passes walk a triangle of W in chunks of CT terms.  The vector operand of a chunk is staged in LDS by the whole
// workgroup (the gather through `rows` runs in parallel and not once per term), the entries of W of APPLY_UNROLL terms
// are loaded before the first of them is used, and the terms are then added in ascending order: the latency of the
// loads is paid once per group of terms and the sum is the sequential one of the statement.
constexpr int APPLY_UNROLL = 16;
static_assert(CT % APPLY_UNROLL == 0, "EQLB_COARSE_TILE");

// y_i = (sum_{k <= i} w_ik r[rows[k]]) / d_i from Wt [k][i]: one thread per row, k ascending, the sum starts from 0.0
template <int NC>
__global__ void __launch_bounds__(CT)
k_coarse_forward(int32_t n, int64_t n0, const ManyCols cols, const int32_t* __restrict__ rows,
                 const double* __restrict__ Wt, const double* __restrict__ d, const double* __restrict__ r,
                 double* __restrict__ y)
{
#pragma clang fp contract(off)
  __shared__ double rs[NC][CT];
  const uint32_t live = cols_live<NC>(cols);
  if (!live)
    return;
  const int t = threadIdx.x;
  const int64_t first = (int64_t)blockIdx.x * CT, i = first + t;
  const int64_t last = first + CT - 1 < n - 1 ? first + CT - 1 : n - 1; // the longest row of the workgroup
  double acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c)
    acc[c] = 0.0;
  for (int64_t k0 = 0; k0 <= last; k0 += CT)
  {
    if (k0 + t <= last)
    {
      const int64_t row = rows[k0 + t];
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (col_on<NC>(live, c))
          rs[c][t] = (row >= 0 && row < n0) ? r[c * n0 + row] : 0.0;
    }
    __syncthreads();
    if (i < n)
      for (int u0 = 0; u0 < CT && k0 + u0 <= i; u0 += APPLY_UNROLL)
      {
        double w[APPLY_UNROLL];
#pragma unroll
        for (int u = 0; u < APPLY_UNROLL; ++u)
          w[u] = k0 + u0 + u <= i ? Wt[(k0 + u0 + u) * n + i] : 0.0;
#pragma unroll
        for (int u = 0; u < APPLY_UNROLL; ++u)
          if (k0 + u0 + u <= i)
          {
#pragma unroll
            for (int c = 0; c < NC; ++c)
              if (col_on<NC>(live, c))
                acc[c] = acc[c] + w[u] * rs[c][u0 + u];
          }
      }
    __syncthreads();
  }
  if (i < n)
  {
    const double di = d[i];
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (col_on<NC>(live, c))
        y[(int64_t)c * n + i] = acc[c] / di;
  }
}

// z[rows[j]] = sum_{i >= j} w_ij y_i from W [i][j]: one thread per column, i ascending, the sum starts from 0.0; then
// every thread of the grid clears its share of the fixed rows
template <int NC>
__global__ void __launch_bounds__(CT)
k_coarse_backward(int32_t n, int64_t n0, const ManyCols cols, const int32_t* __restrict__ rows,
                  const double* __restrict__ W, const double* __restrict__ y, const uint8_t* __restrict__ fixed,
                  double* __restrict__ z)
{
#pragma clang fp contract(off)
  __shared__ double ys[NC][CT];
  const uint32_t live = cols_live<NC>(cols);
  if (!live)
    return;
  const int t = threadIdx.x;
  const int64_t first = (int64_t)blockIdx.x * CT, j = first + t;
  if (first < n) // (the same for the whole workgroup)
  {
    double acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c)
      acc[c] = 0.0;
    for (int64_t i0 = first; i0 < n; i0 += CT)
    {
      if (i0 + t < n)
      {
#pragma unroll
        for (int c = 0; c < NC; ++c)
          if (col_on<NC>(live, c))
            ys[c][t] = y[(int64_t)c * n + i0 + t];
      }
      __syncthreads();
      if (j < n)
        for (int u0 = 0; u0 < CT && i0 + u0 < n; u0 += APPLY_UNROLL)
        {
          double w[APPLY_UNROLL];
#pragma unroll
          for (int u = 0; u < APPLY_UNROLL; ++u)
          {
            const int64_t i = i0 + u0 + u;
            w[u] = (i >= j && i < n) ? W[i * n + j] : 0.0;
          }
#pragma unroll
          for (int u = 0; u < APPLY_UNROLL; ++u)
          {
            const int64_t i = i0 + u0 + u;
            if (i >= j && i < n)
            {
#pragma unroll
              for (int c = 0; c < NC; ++c)
                if (col_on<NC>(live, c))
                  acc[c] = acc[c] + w[u] * ys[c][u0 + u];
            }
          }
        }
      __syncthreads();
    }
    if (j < n)
    {
      const int64_t row = rows[j];
      if (row >= 0 && row < n0)
      {
#pragma unroll
        for (int c = 0; c < NC; ++c)
          if (col_on<NC>(live, c))
            z[c * n0 + row] = acc[c];
      }
    }
  }
  for (int64_t e = (int64_t)blockIdx.x * CT + t; e < n0; e += (int64_t)gridDim.x * CT)
    if (fixed[e])
    {
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (col_on<NC>(live, c))
          z[c * n0 + e] = 0.0;
    }
}
} // namespace

int coarse_setup(const char* who, CoarseSolve& cs, const SolverLevel& lv, hipStream_t stream)
{
  cs.on = 0;
  const int64_t n0 = lv.ndofs * lv.bs;
  // the status word of the mask of level 0 and the mask itself: the call waits by nature
  int32_t status[4] = {0, 0, 0, 0};
  std::vector<uint8_t> fixed((size_t)n0);
  HIP_TRY(hipMemcpyAsync(status, lv.status, sizeof(status), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(fixed.data(), lv.fixed, (size_t)n0, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  for (int c = 0; c < lv.bs; ++c)
    if (status[1 + c] < 1 && !lv.definite(lv.handle))
      return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: singular: component %d of level 0 has no Dirichlet DOF", who, c);
  std::vector<int32_t> rows;
  for (int64_t e = 0; e < n0; ++e)
    if (!fixed[(size_t)e])
      rows.push_back((int32_t)e);
  if (rows.size() > (size_t)COARSE_MAX_ROWS)
    return fail(EQLB_ERR_UNSUPPORTED, "%s: level 0 has %lld free rows, the dense factor takes at most %d", who,
                (long long)rows.size(), COARSE_MAX_ROWS);
  const int32_t n = (int32_t)rows.size();
  if (n > cs.cap)
  {
    cs.cap = -1;
    const size_t nn = (size_t)n * (size_t)n;
    HIP_TRY(cs.rows.alloc_raw((size_t)n));
    HIP_TRY(cs.d.alloc_raw((size_t)n));
    HIP_TRY(cs.W.alloc_raw(nn));
    HIP_TRY(cs.Wt.alloc_raw(nn));
    HIP_TRY(cs.panel.alloc_raw((size_t)n * CB));
    HIP_TRY(cs.y.alloc_raw((size_t)MANY_R * n));
    HIP_TRY(cs.status.alloc_raw(1));
    cs.cap = n;
  }
  cs.n = n;
  cs.n0 = n0;
  if (n == 0)
  {
    cs.on = 1;
    return EQLB_OK;
  }
  HIP_TRY(hipMemcpyAsync(cs.rows.get(), rows.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemsetAsync(cs.status.get(), 0, sizeof(int32_t), stream));
  HIP_TRY(hipMemsetAsync(cs.W.get(), 0, (size_t)n * n * sizeof(double), stream));
  hipLaunchKernelGGL(k_coarse_unit_diagonal, dim3(grid_of(n, UNIT_THREADS)), dim3(UNIT_THREADS), 0, stream, n,
                     cs.W.get());
  HIP_TRY(hipGetLastError());
  // A_0 into Wt, R columns per product of the level-0 handle
  double* const A = cs.Wt.get();
  const int R = lv.bs == 1 ? (n < MANY_R ? n : MANY_R) : 1;
  PcgWork w;
  EQLB_TRY(lv.work(lv.handle, R, w));
  const unsigned unit_grid = grid_of(n0, UNIT_THREADS) < 512u ? grid_of(n0, UNIT_THREADS) : 512u;
  for (int32_t j0 = 0; j0 < n; j0 += R)
  {
    const int Rj = n - j0 < R ? n - j0 : R;
    hipLaunchKernelGGL(k_coarse_units, dim3(unit_grid), dim3(UNIT_THREADS), 0, stream, n0, R, n, j0,
                       static_cast<const int32_t*>(cs.rows.get()), w.d);
    HIP_TRY(hipGetLastError());
    HIP_TRY(lv.product(lv.handle, ManyCols{R, (1u << Rj) - 1u, 0, nullptr}, stream));
    hipLaunchKernelGGL(k_coarse_pick, dim3(grid_of(n, UNIT_THREADS)), dim3(UNIT_THREADS), 0, stream, n0, Rj, n, j0,
                       static_cast<const int32_t*>(cs.rows.get()), static_cast<const double*>(w.q), A);
    HIP_TRY(hipGetLastError());
  }
  for (int32_t k0 = 0; k0 < n; k0 += CB)
  {
    const int32_t nb = n - k0 < CB ? n - k0 : CB, s = k0 + nb;
    hipLaunchKernelGGL(k_coarse_panel, dim3(grid_of(n - k0, CT)), dim3(CT), 0, stream, n, k0, nb, A, cs.panel.get(),
                       cs.d.get(), cs.status.get());
    HIP_TRY(hipGetLastError());
    if (nb > 1)
    {
      hipLaunchKernelGGL(k_coarse_wpanel, dim3(grid_of(s, CT)), dim3(CT), 0, stream, n, k0, nb, cs.W.get(),
                         static_cast<const double*>(cs.panel.get()));
      HIP_TRY(hipGetLastError());
    }
    if (s < n) // (then nb = CB)
    {
      const unsigned below = grid_of(n - s, CT);
      hipLaunchKernelGGL(k_coarse_trail<0>, dim3(below, below), dim3(TRAIL_THREADS), 0, stream, n, k0, A,
                         static_cast<const double*>(cs.panel.get()));
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(k_coarse_trail<1>, dim3(grid_of(s, CT), below), dim3(TRAIL_THREADS), 0, stream, n, k0,
                         cs.W.get(), static_cast<const double*>(cs.panel.get()));
      HIP_TRY(hipGetLastError());
    }
  }
  const unsigned tiles = grid_of(n, CB);
  hipLaunchKernelGGL(k_coarse_transpose, dim3(tiles, tiles), dim3(UNIT_THREADS), 0, stream, n,
                     static_cast<const double*>(cs.W.get()), cs.Wt.get());
  HIP_TRY(hipGetLastError());
  int32_t bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, cs.status.get(), sizeof(bad), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  if (bad != 0)
    return fail(EQLB_ERR_SINGULAR, "%s: singular: pivot %d (row %d of level 0) is not positive", who, (int)bad - 1,
                (int)rows[(size_t)bad - 1]);
  cs.on = 1;
  return EQLB_OK;
}

hipError_t coarse_apply(const CoarseSolve& cs, const ManyCols& c, const double* r, const uint8_t* fixed, double* z,
                        hipStream_t stream)
{
  const int32_t n = cs.n;
  const int64_t n0 = cs.n0;
  const unsigned rows_grid = grid_of(n, CT);
  const unsigned all_grid = grid_of(n0, CT) < 512u ? grid_of(n0, CT) : 512u;
  const dim3 back(rows_grid > all_grid ? rows_grid : (all_grid > 0 ? all_grid : 1u)), block(CT);
  const int32_t* rows = cs.rows.get();
  const double *W = cs.W.get(), *Wt = cs.Wt.get(), *d = cs.d.get();
  double* y = cs.y.get();
  if (c.R == 1)
  {
    if (n > 0)
      hipLaunchKernelGGL(k_coarse_forward<1>, dim3(rows_grid), block, 0, stream, n, n0, c, rows, Wt, d, r, y);
    hipLaunchKernelGGL(k_coarse_backward<1>, back, block, 0, stream, n, n0, c, rows, W, static_cast<const double*>(y),
                       fixed, z);
  }
  else
  {
    if (n > 0)
      hipLaunchKernelGGL(k_coarse_forward<MANY_R>, dim3(rows_grid), block, 0, stream, n, n0, c, rows, Wt, d, r, y);
    hipLaunchKernelGGL(k_coarse_backward<MANY_R>, back, block, 0, stream, n, n0, c, rows, W,
                       static_cast<const double*>(y), fixed, z);
  }
  return hipGetLastError();
}
} // namespace eqlb
