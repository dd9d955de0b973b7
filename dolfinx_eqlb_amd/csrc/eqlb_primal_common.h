// What the P_p Poisson solve (eqlb_primal_solve.hip), the P_p^2 elasticity solve (eqlb_primal_elasticity.hip) and the
// hierarchy (eqlb_multilevel.hip) share: the sum pass of the store-and-sum operator, the vector kernels and the scalar
// kernel of the preconditioned CG, and the host loop that drives them - ONE implementation for 1 ... MANY_R right-hand
// sides (eqlb_*_many of include/eqlb.h); the single-vector entries are its one-column callers.  Everything lies in an
// unnamed namespace: each unit gets its own copy.
// THE RULE: column c of a many-solve is the single solve of (b_c, u_c) - the same bits, the same info.  What makes it hold:
//  - one thread per DOF carries the values of that DOF in all columns: the grid is stream_blocks(n), the per-thread
//    order over the DOFs and the block tree do not depend on the columns, so every inner product of a column is the
//    same sum whatever runs beside it.  Block partials [R][2][G];
//  - every column has its own PcgState; a kernel works on the columns of its ManyCols (eqlb_internal.h) and leaves the
//    others alone, so a column freezes at its stop flag while the others go on, and waits untouched for the host;
//  - k_pcg_scalar runs one block per column.
// Vectors are [R][n], one column after another (the layout eqlb_primal_flux_dg and eqlb_refine_prolong_lagrange read);
// R <= MANY_R columns per group, a larger count runs group after group.  The column slots of a kernel are its template
// parameter NC (arrays [NC], shared [NC or 2 NC][PS_THREADS]): NC = 1 serves one column, NC = MANY_R two to four.
//  k_primal_slots    builds the slot lists of the sum pass once at create (scalar numbering: both problems use it)
//  k_primal_mask<BS> the Dirichlet mask of one component from a list of facets
//  k_primal_gather<BS, NC>  one thread per (DOF, component): BS values per y_loc entry, the vectors blocked
//                    x[BS * dof + r]; columns for BS = 1 only.  eqlb_primal_gather.inc, included twice: the second
//                    time as k_primal_gather_facet, which adds the facet values of a Robin term (BS = 1) or a spring
//                    term (BS = 2)
//  k_pcg_*<NC>       work on any length n with a byte mask [n]: n = ndofs or 2 ndofs
//  k_pcg_scalar      the scalar steps; `ml`: the breakdown rule of a preconditioner that is no positive diagonal
//  pcg_solve         the host side of the iteration on a PcgWork; the preconditioner enters through its `steps`
//                    (JacobiSteps here; the hierarchy unit eqlb_multilevel.hip brings its own)
// The host side of the two solver handles on these kernels (the handle base, its launches, the bodies of the C entries)
// lies in eqlb_primal_handle.h.
#pragma once

#include "eqlb_device_common.h"
#include "eqlb_facet_plan.h"
#include "eqlb_host_util.h"
#include "eqlb_reduce.h"

#include <cstdint>

namespace eqlb
{
namespace
{
constexpr int PS_THREADS = 256;
constexpr int PS_MAXBLOCKS = 512; // blocks of a streaming kernel over the DOFs
constexpr int PS_PMAX = 4, PS_DMAX = 3;
constexpr int PRIMAL_CHECK_EVERY = EQLB_PRIMAL_CHECK_EVERY;
static_assert(PRIMAL_CHECK_EVERY >= 1, "EQLB_PRIMAL_CHECK_EVERY");

enum CellMode
{
  CELL_OPERATOR = 0,
  CELL_DIAGONAL = 1,
  CELL_LOAD = 2
};

// the shapes of the space and the tables of the sum pass
struct SpaceArgs
{
  int64_t ndofs;
  int32_t nnodes, nfacets, ncells, ne, ni, nd;
  const int32_t *nco, *fco; // offsets of node -> cell, facet -> cell
  const int32_t* slots;     // [3 ncells (1 + ne)] flat indices c * nd + i into y_loc
};

__host__ __device__ inline int stream_blocks(int64_t n)
{
  const int64_t b = (n + PS_THREADS - 1) / PS_THREADS;
  return (int)(b < PS_MAXBLOCKS ? (b < 1 ? 1 : b) : PS_MAXBLOCKS);
}

// first slot and number of slots of the vertex or facet DOF d < nnodes + nfacets * ne
__device__ __forceinline__ void slot_range(const SpaceArgs& s, int64_t d, int64_t& beg, int& cnt)
{
  if (d < s.nnodes)
  {
    beg = s.nco[d];
    cnt = s.nco[d + 1] - s.nco[d];
  }
  else
  {
    const int64_t q = d - s.nnodes, f = q / s.ne;
    const int j = (int)(q - f * s.ne);
    cnt = s.fco[f + 1] - s.fco[f];
    beg = 3 * (int64_t)s.ncells + (int64_t)s.fco[f] * s.ne + (int64_t)j * cnt;
  }
}

// one thread per vertex / facet DOF: its slots in the order of the node -> cell / facet -> cell table; the local index
// comes from matching ids.  A cell that does not hold the DOF (a broken table) gets its entry 0 and is counted
__global__ void __launch_bounds__(PS_THREADS)
k_primal_slots(const SpaceArgs s, const int32_t* __restrict__ node_cells, const int32_t* __restrict__ facet_cells,
               const int32_t* __restrict__ cell_dofs, int32_t* __restrict__ slots, int32_t* __restrict__ status)
{
  const int64_t d = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  const int64_t nshared = (int64_t)s.nnodes + (int64_t)s.nfacets * s.ne;
  if (d >= nshared)
    return;
  int64_t beg;
  int cnt;
  slot_range(s, d, beg, cnt);
  const int32_t* cells = d < s.nnodes ? node_cells + s.nco[d] : facet_cells + s.fco[(d - s.nnodes) / s.ne];
  for (int k = 0; k < cnt; ++k)
  {
    const int64_t c = cells[k];
    int loc = -1;
    for (int i = 0; i < s.nd; ++i)
      loc = (cell_dofs[c * s.nd + i] == (int32_t)d) ? i : loc;
    if (loc < 0)
    {
      atomicAdd(status + 2, 1);
      loc = 0;
    }
    slots[beg + k] = (int32_t)(c * s.nd + loc);
  }
}

// the mask of component r: the rows BS dof + r of the vertex and facet DOFs of the listed facets; ids outside the mesh are
// skipped and counted (status[0]), valid ones counted per component (status[1 + r])
template <int BS>
__global__ void __launch_bounds__(PS_THREADS)
k_primal_mask(int32_t nlist, const int32_t* __restrict__ facets, int32_t r, int32_t nnodes, int32_t nfacets, int32_t ne,
              const int32_t* __restrict__ facet_nodes, uint8_t* __restrict__ fixed, int32_t* __restrict__ status)
{
  const int32_t i = blockIdx.x * PS_THREADS + threadIdx.x;
  if (i >= nlist)
    return;
  const int32_t f = facets[i];
  if (f < 0 || f >= nfacets)
  {
    atomicAdd(status, 1);
    return;
  }
  atomicAdd(status + 1 + r, 1);
  fixed[BS * (int64_t)facet_nodes[2 * (int64_t)f] + r] = 1;
  fixed[BS * (int64_t)facet_nodes[2 * (int64_t)f + 1] + r] = 1;
  for (int j = 0; j < ne; ++j)
    fixed[BS * ((int64_t)nnodes + (int64_t)f * ne + j) + r] = 1;
}

enum GatherDot
{
  DOT_NONE = 0,
  DOT_W_Y = 1, // sum_d w[d] y[d]
  DOT_R_R = 2  // sum_d r[d]^2
};

struct GatherArgs
{
  SpaceArgs s;
  const double* yloc;   // column c: yloc + c * ystride
  const uint8_t* fixed; // nullptr: the raw operator
  const double* add;    // nullptr or b_extra (one column)
  const double* b;      // with r: r = b - sum (0 on fixed rows)
  const double* w;      // DOT_W_Y
  double *y, *r;        // each nullptr or column 0 of [R][BS ndofs]; so are b, w
  double* part;         // [R][2][gridDim.x] block partials of the inner product: channel 0 is written
  int32_t dot;
  ManyCols cols;
  int64_t ystride;
};

// the launch of a streaming kernel template on the columns of c: the one-column instance or the MANY_R-column one.
// MAXC = 1 (inside a template: the steps of a unit whose handles hold one column) instantiates no wider kernel
#define EQLB_LAUNCH_COLS(MAXC, KERNEL, R, n, stream, ...)                                                              \
  do                                                                                                                   \
  {                                                                                                                    \
    if constexpr ((MAXC) == 1)                                                                                         \
      hipLaunchKernelGGL(KERNEL<1>, dim3(stream_blocks(n)), dim3(PS_THREADS), 0, stream, __VA_ARGS__);                 \
    else if ((R) == 1)                                                                                                 \
      hipLaunchKernelGGL(KERNEL<1>, dim3(stream_blocks(n)), dim3(PS_THREADS), 0, stream, __VA_ARGS__);                 \
    else                                                                                                               \
      hipLaunchKernelGGL(KERNEL<MANY_R>, dim3(stream_blocks(n)), dim3(PS_THREADS), 0, stream, __VA_ARGS__);            \
  } while (0)

// A facet term of the sum pass, all pointers DEVICE: the Robin term of a scalar space (include/eqlb.h:
// eqlb_primal_set_robin) or the spring term of a blocked one, bs = 2 (eqlb_elasticity_set_springs).  The table a row
// finds its facets through (eqlb_facet_plan.h) runs over the scalar DOFs d - with bs = 2 both rows 2 d + r of a DOF lie
// in the same facets, and a chunk of PS_THREADS consecutive rows holds PS_THREADS / 2 consecutive DOFs.  A kernel
// argument of its own, which the sum pass without the term does not take.
static_assert(FACET_ROW == PS_PMAX + 1, "the p + 1 rows of a facet in its local order");
struct FacetTermArgs
{
  const int32_t* chunk; // [ceil(bs ndofs / PS_THREADS) + 1] first position in rows[] of a chunk of PS_THREADS / bs DOFs
  const int32_t* rows;  // [m] the DOFs that lie in a listed facet, ascending
  const int32_t* off;   // [m + 1] the entries of a DOF in ent[]
  const int32_t* ent;   // list position * 8 + local index of the DOF in that facet, facet ids ascending
  const int32_t* dofs;  // [nlist][FACET_ROW], scalar DOFs
  const double* w;      // bs = 1: [nlist] alpha_f |E_f|; bs = 2: [nlist][3] |E_f| (k00, k01, k11)
  const double* fm;     // FacetMass<p> [n1][n1]
  const double* u;      // column 0 of [R][bs ndofs], blocked; nullptr: the diagonal
  const uint8_t* fixed; // [bs ndofs]; only_fixed: the free rows of u read as 0
  int32_t only_fixed, n1;
};

#define EQLB_GATHER_FACET 0
#include "eqlb_primal_gather.inc"
#undef EQLB_GATHER_FACET
#define EQLB_GATHER_FACET 1
#include "eqlb_primal_gather.inc"
#undef EQLB_GATHER_FACET

// ---- vector kernels of the iteration (grid-stride, block partials in a fixed order): the columns of a DOF in one
// thread.  Channel j of column k: sh[2 k + j], part[(2 k + j) G + block] ----------------------------------------------
// z = r / diag on the free rows (0 on the fixed ones); partials of r.r and r.z: channels 0 and 1
template <int NC>
__global__ void __launch_bounds__(PS_THREADS)
k_pcg_precond(int64_t n, const ManyCols cols, const double* __restrict__ r, const double* __restrict__ diag,
              const uint8_t* __restrict__ fixed, double* __restrict__ z, double* __restrict__ part)
{
#pragma clang fp contract(off)
  __shared__ double sh[2 * NC][PS_THREADS];
  const uint32_t live = cols_live<NC>(cols);
  if (!live)
    return;
  const int t = threadIdx.x, G = gridDim.x;
  double a0[NC], a1[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k)
    a0[k] = a1[k] = 0.0;
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + t; d < n; d += (int64_t)G * PS_THREADS)
  {
    const bool fx = fixed[d];
    const double dg = diag[d];
#pragma unroll
    for (int k = 0; k < NC; ++k)
    {
      if (!col_on<NC>(live, k))
        continue;
      const double rv = r[k * n + d], zv = fx ? 0.0 : rv / dg;
      z[k * n + d] = zv;
      a0[k] = a0[k] + rv * rv;
      a1[k] = a1[k] + rv * zv;
    }
  }
#pragma unroll
  for (int k = 0; k < NC; ++k)
  {
    sh[2 * k][t] = a0[k];
    sh[2 * k + 1][t] = a1[k];
  }
  __syncthreads();
  EQLB_BLOCK_TREE_SUM(sh, t, 2 * NC, PS_THREADS)
  if (t < 2 * NC && col_on<NC>(live, t / 2))
    part[(int64_t)t * G + blockIdx.x] = sh[t][0];
}

// u += alpha p, r -= alpha q, z = r / diag on the free rows; the fixed rows are not touched; partials as k_pcg_precond
template <int NC>
__global__ void __launch_bounds__(PS_THREADS)
k_pcg_update(int64_t n, const ManyCols cols, const double* __restrict__ p, const double* __restrict__ q,
             const double* __restrict__ diag, const uint8_t* __restrict__ fixed, double* __restrict__ u,
             double* __restrict__ r, double* __restrict__ z, double* __restrict__ part)
{
#pragma clang fp contract(off)
  __shared__ double sh[2 * NC][PS_THREADS];
  const uint32_t live = cols_live<NC>(cols);
  if (!live)
    return;
  const int t = threadIdx.x, G = gridDim.x;
  double alpha[NC], a0[NC], a1[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k)
  {
    alpha[k] = col_on<NC>(live, k) ? cols.st[k].alpha : 0.0;
    a0[k] = a1[k] = 0.0;
  }
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + t; d < n; d += (int64_t)G * PS_THREADS)
  {
    if (fixed[d])
      continue; // (r and z are 0 there since the start)
    const double dg = diag[d];
#pragma unroll
    for (int k = 0; k < NC; ++k)
    {
      if (!col_on<NC>(live, k))
        continue;
      const int64_t e = k * n + d;
      u[e] = u[e] + alpha[k] * p[e];
      const double rv = r[e] - alpha[k] * q[e], zv = rv / dg;
      r[e] = rv;
      z[e] = zv;
      a0[k] = a0[k] + rv * rv;
      a1[k] = a1[k] + rv * zv;
    }
  }
#pragma unroll
  for (int k = 0; k < NC; ++k)
  {
    sh[2 * k][t] = a0[k];
    sh[2 * k + 1][t] = a1[k];
  }
  __syncthreads();
  EQLB_BLOCK_TREE_SUM(sh, t, 2 * NC, PS_THREADS)
  if (t < 2 * NC && col_on<NC>(live, t / 2))
    part[(int64_t)t * G + blockIdx.x] = sh[t][0];
}

// p = z + beta p (first: p = z)
template <int NC>
__global__ void __launch_bounds__(PS_THREADS)
k_pcg_direction(int64_t n, const ManyCols cols, int first, const double* __restrict__ z, double* __restrict__ p)
{
#pragma clang fp contract(off)
  const uint32_t live = cols_live<NC>(cols);
  if (!live)
    return;
  double beta[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k)
    beta[k] = (!first && col_on<NC>(live, k)) ? cols.st[k].beta : 0.0;
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x; d < n; d += (int64_t)gridDim.x * PS_THREADS)
  {
#pragma unroll
    for (int k = 0; k < NC; ++k)
    {
      if (!col_on<NC>(live, k))
        continue;
      const int64_t e = k * n + d;
      p[e] = first ? z[e] : z[e] + beta[k] * p[e];
    }
  }
}

// u = u^: the free rows set to 0 (nothing to solve)
template <int NC>
__global__ void __launch_bounds__(PS_THREADS)
k_pcg_clear_free(int64_t n, const ManyCols cols, const uint8_t* __restrict__ fixed, double* __restrict__ u)
{
  const uint32_t live = cols_live<NC>(cols);
  if (!live)
    return;
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x; d < n; d += (int64_t)gridDim.x * PS_THREADS)
    if (!fixed[d])
    {
#pragma unroll
      for (int k = 0; k < NC; ++k)
        if (col_on<NC>(live, k))
          u[k * n + d] = 0.0;
    }
}

enum ScalarStep
{
  STEP_NORM = 0,    // out[0] = sqrt(channel 0); knows no state
  STEP_NB = 1,      // nb = sqrt(channel 0), tol = max(rtol nb, atol)
  STEP_START = 2,   // rr, rho from the start residual; done if it is within tol already
  STEP_ALPHA = 3,   // pq = channel 0: breakdown unless > 0, else alpha = rho / pq
  STEP_BETA = 4,    // rr, rho_new: one more iteration done; done if sqrt(rr) <= tol, else beta, rho
  STEP_TRUE = 5,    // rtrue = sqrt(channel 0); converged if <= tol
  STEP_REPLACE = 6  // after the true residual replaced r: beta = rho_new / rho, rho = rho_new, the iteration goes on
};

// One block per column: block k forms the channels' totals over the G block partials of column k by the same tree,
// then its thread 0 moves the state of column k.  mask picks the columns; the stop flag is looked at per step.  ml: the
// preconditioner is no positive diagonal - breakdown where the iteration would go on with r.z <= 0 or NaN
__global__ void __launch_bounds__(PS_THREADS)
k_pcg_scalar(int step, int ml, int G, uint32_t mask, const double* __restrict__ part_, PcgState* __restrict__ st_,
             double rtol, double atol, double* __restrict__ out)
{
  __shared__ double sh[2][PS_THREADS];
  const int t = threadIdx.x;
  if (!((mask >> blockIdx.x) & 1u))
    return;
  PcgState* st = st_ + blockIdx.x; // (not read at STEP_NORM)
  const double* part = part_ + (int64_t)blockIdx.x * 2 * G;
  const bool two = step == STEP_START || step == STEP_BETA || step == STEP_REPLACE;
  if (step != STEP_NORM && step != STEP_TRUE && step != STEP_REPLACE && st->done)
    return;
#pragma unroll
  for (int j = 0; j < 2; ++j)
  {
    double a = 0.0;
    if (j == 0 || two)
      for (int b = t; b < G; b += PS_THREADS)
        a += part[(int64_t)j * G + b];
    sh[j][t] = a;
  }
  __syncthreads();
  EQLB_BLOCK_TREE_SUM(sh, t, 2, PS_THREADS)
  if (t != 0)
    return;
  const double s0 = sh[0][0], s1 = sh[1][0];
  bool goes_on = two; // the iteration goes on with s1 as its r.z
  switch (step)
  {
  case STEP_NORM:
    out[0] = sqrt(s0);
    break;
  case STEP_NB:
    st->nb = sqrt(s0);
    st->tol = fmax(rtol * st->nb, atol);
    break;
  case STEP_START:
    st->rr = s0;
    st->rho = s1;
    if (sqrt(s0) <= st->tol)
    {
      st->done = 1;
      goes_on = false;
    }
    break;
  case STEP_ALPHA:
    st->pq = s0;
    if (!(s0 > 0.0))
    {
      st->breakdown = 1;
      st->done = 1;
    }
    else
      st->alpha = st->rho / s0;
    break;
  case STEP_BETA:
    st->rr = s0;
    st->iters += 1;
    if (sqrt(s0) <= st->tol)
    {
      st->done = 1; // (rho stays that of the last direction: STEP_REPLACE needs it if the true residual is above tol)
      goes_on = false;
    }
    else
    {
      st->beta = s1 / st->rho;
      st->rho = s1;
    }
    break;
  case STEP_TRUE:
    st->rtrue = sqrt(s0);
    st->converged = (st->rtrue <= st->tol) ? 1 : 0;
    break;
  default: // STEP_REPLACE
    st->rr = s0;
    st->beta = s1 / st->rho;
    st->rho = s1;
    st->replacements += 1;
    st->done = 0;
  }
  if (ml && goes_on && !(s1 > 0.0))
  {
    st->breakdown = 1;
    st->done = 1;
  }
}

// ---- host side of the iteration ------------------------------------------------------------------------------------
inline ManyCols work_cols(const PcgWork& w, uint32_t mask, bool check)
{
  return ManyCols{w.R, mask, check ? 1 : 0, w.st};
}

// the scalar step on the columns of mask (STEP_NORM: the total of column 0 into out, no state)
inline hipError_t launch_scalar(const PcgWork& w, uint32_t mask, int step, int ml, double rtol, double atol, double* out,
                                hipStream_t stream)
{
  hipLaunchKernelGGL(k_pcg_scalar, dim3(w.R), dim3(PS_THREADS), 0, stream, step, ml, stream_blocks(w.n), mask,
                     static_cast<const double*>(w.part), w.st, rtol, atol, out);
  return hipGetLastError();
}

// The two places where the preconditioner enters the iteration, for z = r / diag: both kernels fuse it
template <int MAXC> // the columns the handles of the unit hold at the most: 1 or MANY_R
struct JacobiSteps
{
  static constexpr int max_cols = MAXC;
  static constexpr int check_every = PRIMAL_CHECK_EVERY; // iterations between two reads of the states by the host
  const PcgWork& w;
  hipStream_t stream;
  // z from the r of the start or of a replacement, the partials of r.r and r.z, the scalar step (STEP_START / _REPLACE)
  hipError_t restart(const ManyCols& c, int step, double rtol, double atol) const
  {
    EQLB_LAUNCH_COLS(MAXC, k_pcg_precond, w.R, w.n, stream, w.n, c, static_cast<const double*>(w.r), w.diag, w.fixed, w.z,
                     w.part);
    return launch_scalar(w, c.mask, step, 0, rtol, atol, nullptr, stream);
  }
  // u += alpha d, r -= alpha q, z from the new r, the partials of r.r and r.z, STEP_BETA
  hipError_t advance(const ManyCols& c, double* pu, double rtol, double atol) const
  {
    EQLB_LAUNCH_COLS(MAXC, k_pcg_update, w.R, w.n, stream, w.n, c, static_cast<const double*>(w.d),
                     static_cast<const double*>(w.q), w.diag, w.fixed, pu, w.r, w.z, w.part);
    return launch_scalar(w, c.mask, STEP_BETA, 0, rtol, atol, nullptr, stream);
  }
};

// The preconditioned CG of eqlb_primal_solve / eqlb_elasticity_solve / eqlb_hierarchy_solve and their _many forms behind
// the argument checks, column by column, for one group of w.R <= MANY_R columns; b, u DEVICE [R][n], info HOST [R][8].
//   residual(cols, b, u, r, only_fixed)  enqueues r = b - A u (0 on the fixed rows; u^ instead of u with only_fixed) on
//                                        the columns of `cols` and leaves the block partials of r.r in w.part
//   product(cols)                        enqueues q = A d on the free rows with the block partials of d.q in w.part
//   steps                                the preconditioner: restart(cols, step, rtol, atol) and
//                                        advance(cols, u, rtol, atol) as JacobiSteps
// skipped: the facet ids the mask skipped (info[7]).
// At each read of the states the columns whose flag is set get the true residual; of these the ones above tolerance get
// the replacement and the restart, alone; a column that has converged, broken down or reached maxit is retired and no
// later launch names it.  Inside a batch a column stops at its own flag, so the batch may be sized by the live column
// with the fewest iterations left: the others go on in the next one.
template <class Residual, class Product, class Steps>
int pcg_solve(const PcgWork& w, Residual&& residual, Product&& product, const Steps& steps, const double* pb, double* pu,
              double rtol, double atol, int32_t maxit, double* info, int32_t skipped, hipStream_t stream)
{
  const int R = w.R;
  const uint32_t all = (1u << R) - 1u;
  PcgState hs[MANY_R]{}, tmp[MANY_R]{};
  bool have_true[MANY_R] = {false, false, false, false}; // q holds the true residual of the column's u, the state its norm
  hipError_t err = hipSuccess;
  auto note = [&](hipError_t e) {
    if (err == hipSuccess)
      err = e;
  };
  auto in = [](uint32_t mask, int c) { return ((mask >> c) & 1u) != 0; };
  auto read_states = [&](uint32_t mask) {
    note(hipMemcpyAsync(tmp, w.st, (size_t)R * sizeof(PcgState), hipMemcpyDeviceToHost, stream));
    note(hipStreamSynchronize(stream));
    for (int c = 0; c < R && err == hipSuccess; ++c)
      if (in(mask, c))
        hs[c] = tmp[c];
  };
  auto true_residual = [&](uint32_t mask) {
    note(residual(work_cols(w, mask, false), pb, pu, w.q, false));
    note(launch_scalar(w, mask, STEP_TRUE, 0, rtol, atol, nullptr, stream));
  };
  auto direction = [&](uint32_t mask, int first) {
    EQLB_LAUNCH_COLS(Steps::max_cols, k_pcg_direction, R, w.n, stream, w.n, work_cols(w, mask, true), first,
                     static_cast<const double*>(w.z), w.d);
    note(hipGetLastError());
  };
  note(hipMemsetAsync(w.st, 0, (size_t)R * sizeof(PcgState), stream));
  note(residual(work_cols(w, all, false), pb, pu, w.q, true));
  note(launch_scalar(w, all, STEP_NB, 0, rtol, atol, nullptr, stream));
  note(residual(work_cols(w, all, false), pb, pu, w.r, false));
  note(steps.restart(work_cols(w, all, false), STEP_START, rtol, atol));
  direction(all, 1);
  read_states(all);
  uint32_t live = all, nothing = 0;
  for (int c = 0; c < R; ++c)
    if (hs[c].tol == 0.0 && hs[c].nb == 0.0)
      nothing |= 1u << c;
  if (err == hipSuccess && nothing)
  {
    // nothing to solve in these columns: u^ is the solution
    EQLB_LAUNCH_COLS(Steps::max_cols, k_pcg_clear_free, R, w.n, stream, w.n, work_cols(w, nothing, false), w.fixed, pu);
    note(hipGetLastError());
    for (int c = 0; c < R; ++c)
      if (in(nothing, c))
      {
        hs[c].converged = 1;
        hs[c].rtrue = 0.0;
        have_true[c] = true;
      }
    live &= ~nothing;
  }
  // Every pass ends with a batch in which each live column takes at least one iteration or raises its flag for good
  // (breakdown), and a column is retired at iters >= maxit: maxit passes at the most, and two for the ends.  With no
  // replacement it is ceil(maxit / check_every) passes.
  const int max_passes = maxit + 2;
  for (int pass = 0; pass < max_passes && err == hipSuccess && live; ++pass)
  {
    uint32_t flagged = 0;
    for (int c = 0; c < R; ++c)
      if (in(live, c))
      {
        if (hs[c].breakdown || hs[c].converged)
          live &= ~(1u << c);
        else if (hs[c].done)
          flagged |= 1u << c;
      }
    if (flagged)
    {
      // the recurrence residual of these columns reached tol: the true one decides
      true_residual(flagged);
      read_states(flagged);
      uint32_t replace = 0;
      for (int c = 0; c < R; ++c)
        if (in(flagged, c))
        {
          have_true[c] = true;
          if (hs[c].converged || hs[c].iters >= maxit)
            live &= ~(1u << c);
          else
            replace |= 1u << c;
        }
      if (replace)
      {
        for (int c = 0; c < R; ++c)
          if (in(replace, c))
          {
            note(hipMemcpyAsync(w.r + c * w.n, w.q + c * w.n, (size_t)w.n * sizeof(double), hipMemcpyDeviceToDevice,
                                stream));
            have_true[c] = false;
          }
        note(steps.restart(work_cols(w, replace, false), STEP_REPLACE, rtol, atol));
        direction(replace, 0);
      }
    }
    int batch = Steps::check_every;
    for (int c = 0; c < R; ++c)
      if (in(live, c))
      {
        if (hs[c].iters >= maxit)
          live &= ~(1u << c);
        else if (maxit - hs[c].iters < batch)
          batch = maxit - hs[c].iters;
      }
    if (!live)
      break;
    const ManyCols cols = work_cols(w, live, true);
    for (int it = 0; it < batch; ++it)
    {
      note(product(cols));
      note(launch_scalar(w, live, STEP_ALPHA, 0, rtol, atol, nullptr, stream));
      note(steps.advance(cols, pu, rtol, atol));
      direction(live, 0);
    }
    for (int c = 0; c < R; ++c)
      if (in(live, c))
        have_true[c] = false;
    read_states(live);
  }
  uint32_t last = 0;
  for (int c = 0; c < R; ++c)
    if (!have_true[c])
      last |= 1u << c;
  if (last)
  {
    int conv[MANY_R];
    for (int c = 0; c < R; ++c)
      conv[c] = hs[c].converged;
    true_residual(last);
    read_states(last);
    for (int c = 0; c < R; ++c)
      hs[c].converged = conv[c]; // (a run that ended at maxit or broke down is not converged, whatever its last residual)
  }
  HIP_TRY(err);
  for (int c = 0; c < R; ++c)
  {
    double* o = info + 8 * c;
    o[0] = (double)hs[c].iters;
    o[1] = (double)hs[c].converged;
    o[2] = hs[c].nb;
    o[3] = hs[c].rtrue;
    o[4] = (double)hs[c].replacements;
    o[5] = (double)hs[c].breakdown;
    o[6] = hs[c].tol;
    o[7] = (double)skipped;
  }
  return EQLB_OK;
}

// b, u [nrhs][n] of a solve entry, staged when they lie in host memory, handed to `group(R, b, u, info)` in groups of
// R <= MANY_R columns (DEVICE pointers; info HOST [R][8]); u is copied back at the end
template <class Group>
int pcg_solve_groups(int64_t n_, int32_t nrhs, const double* b, double* u, double* info, bool host, hipStream_t stream,
                     Group&& group)
{
  const size_t n = (size_t)n_;
  HostCall s;
  const auto d_b = s.in(host ? b : nullptr, nrhs * n);
  const auto d_u = s.in(host ? static_cast<const double*>(u) : nullptr, nrhs * n);
  if (host)
    HIP_TRY(s.upload(stream));
  const double* pb = host ? d_b.get() : b;
  double* pu = host ? d_u.get() : u;
  for (int32_t c0 = 0; c0 < nrhs; c0 += MANY_R)
    EQLB_TRY(group(nrhs - c0 < MANY_R ? (int)(nrhs - c0) : MANY_R, pb + c0 * n, pu + c0 * n, info + 8 * (size_t)c0));
  if (host)
    s.out_prefix(u, d_u, nrhs * n);
  HIP_TRY(s.finish(stream));
  return EQLB_OK;
}
} // namespace
} // namespace eqlb
