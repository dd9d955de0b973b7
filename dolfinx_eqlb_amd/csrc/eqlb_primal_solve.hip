// The P_p Poisson problem -div(kappa grad u) = f ON THE DEVICE: the operator applied matrix-free on the handle's own
// P_p space (the numbering of eqlb_mesh_lagrange_dofmap), the load vector from DG_d data, the residual of a given u_h
// and a Jacobi-preconditioned CG - the primal solves of the reference's adaptive demos (demo/poisson_adaptive/
// demo_lshape.py, demo_discont-coeff.py, demo/poisson/demo_reconstruction.py), which no DOLFINx can do on a mesh that
// was refined on the device.  The rule is stated in include/eqlb.h and, as numpy, in dolfinx_eqlb_amd/lsolver/primal.py;
// operator, load, diagonal and residual reproduce the numpy statement bit for bit.
//
// The operator is a store pass plus a per-destination sum pass - no atomics, one fixed order of operations per value:
//  k_primal_cell<P, MODE, D>  one thread per cell, PS_THREADS cells per workgroup.  The table (Stiff<P>: 675 doubles,
//    5.4 KB at P = 4; Load<P, D>) is staged in LDS once per workgroup and read as a broadcast; the index rows of the
//    workgroup's cells are read as one contiguous piece and handed out through LDS; the nd_p values of a cell are
//    staged in LDS (odd row stride: no bank conflict of the thread-per-row writes) and written as the contiguous piece
//    of y_loc [ncells][nd_p] the workgroup owns.  MODE: operator, diagonal, load.  Contraction is switched off: the
//    statement rounds every product and every sum on its own.
//  k_primal_gather            one thread per DOF: the sum of its y_loc entries in the order of the slot lists.  The
//    lists of the vertex and facet DOFs lie where the node -> cell and facet -> cell tables put them (vertex n:
//    [nco[n], nco[n+1]); facet DOF (f, j): 3 ncells + fco[f] (p-1) + j cnt_f), so they need no offsets of their own;
//    an interior DOF reads its one entry.  The Dirichlet mask is applied here (a fixed row gives 0), b_extra is added
//    here, r = b - y is fused here, and so is the per-block partial of an inner product with the result.
//  k_primal_slots             builds the lists once at create: the local index comes from matching ids.
// CG: the axpy forms and z = r / diag are streaming kernels over the DOFs; inner products are per-thread partials in a
// fixed order, one tree per block (eqlb_reduce.h), then one block over the block partials (k_pcg_scalar), which also
// forms alpha, beta, rho and the stop flag IN DEVICE MEMORY (PcgState) for the next kernel.  Once the flag is set the
// remaining kernels of a batch return at once, so the result does not depend on how often the host looks: it reads
// the state every EQLB_PRIMAL_CHECK_EVERY iterations.  Nothing is allocated inside the iteration.
#include "eqlb_device_common.h"
#include "eqlb_mesh_handle.h" // (eqlb_host_util.h)
#include "eqlb_reduce.h"
#include "eqlb_tables_gen.h"

#include <climits>
#include <cmath>

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

// scalars of the iteration, in device memory
struct PcgState
{
  double rho, pq, alpha, beta, rr, nb, tol, rtrue;
  int32_t iters, done, breakdown, converged, replacements, pad;
};

struct CellArgs
{
  int32_t ncells;
  const int32_t* cell_dofs; // [ncells][nd_p]
  const double *cellJ, *coeff;
  const double* u;      // operator: [ndofs]; load: rhs_dg [ncells][nd_d]
  const uint8_t* fixed; // operator, only_fixed: the free rows of u read as 0
  int32_t only_fixed;
  double* yloc; // [ncells][nd_p]
  const PcgState* st;
};

template <int P, int MODE, int D>
__global__ void __launch_bounds__(PS_THREADS) k_primal_cell(const CellArgs a)
{
#pragma clang fp contract(off) // the statement rounds every product and every sum on its own
  constexpr int NP = nd_of(P), ND = nd_of(D), S = NP | 1;
  constexpr int NTAB = (MODE == CELL_LOAD) ? NP * ND : 3 * NP * NP;
  static_assert(eqlb_tables::Stiff<P>::ND == NP && eqlb_tables::Load<P, D>::NP == NP && eqlb_tables::Load<P, D>::ND == ND,
                "table shape");
  __shared__ double sT[NTAB];
  __shared__ double sbuf[PS_THREADS * S]; // first the index rows of the workgroup, then its output rows
  if (a.st && a.st->done)
    return;
  const int t = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * PS_THREADS;
  const int nloc = (a.ncells - base < PS_THREADS) ? (int)(a.ncells - base) : PS_THREADS;
  const bool active = t < nloc;
  for (int i = t; i < NTAB; i += PS_THREADS)
  {
    if constexpr (MODE == CELL_LOAD)
      sT[i] = eqlb_tables::Load<P, D>::LD[i];
    else
      sT[i] = eqlb_tables::Stiff<P>::ST[i];
  }
  [[maybe_unused]] int32_t idx[NP];
  if constexpr (MODE == CELL_OPERATOR)
  {
    int32_t* sidx = reinterpret_cast<int32_t*>(sbuf);
    const int32_t* rows = a.cell_dofs + base * NP;
    for (int e = t; e < nloc * NP; e += PS_THREADS)
      sidx[e] = rows[e];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NP; ++i)
      idx[i] = active ? sidx[t * NP + i] : 0;
  }
  __syncthreads(); // the table is staged; the index rows are in registers: sbuf takes the output rows
  if (active)
  {
    const double2* Jp = reinterpret_cast<const double2*>(a.cellJ + 4 * (base + t));
    const double2 r0 = Jp[0], r1 = Jp[1]; // J00 J01 | J10 J11
    const double det = r0.x * r1.y - r0.y * r1.x;
    const double adet = fabs(det);
    if constexpr (MODE == CELL_LOAD)
    {
      const double* f = a.u + (base + t) * ND;
      double fv[ND];
#pragma unroll
      for (int n = 0; n < ND; ++n)
        fv[n] = f[n];
#pragma unroll
      for (int i = 0; i < NP; ++i)
      {
        double s = sT[i * ND] * fv[0];
#pragma unroll
        for (int n = 1; n < ND; ++n)
          s = s + sT[i * ND + n] * fv[n];
        sbuf[t * S + i] = adet * s;
      }
    }
    else
    {
      const double idet = 1.0 / det;
      const double K00 = r1.y * idet, K01 = -r0.y * idet, K10 = -r1.x * idet, K11 = r0.x * idet;
      const double C00 = K00 * K00 + K01 * K01, C01 = K00 * K10 + K01 * K11, C11 = K10 * K10 + K11 * K11;
      const double w = (a.coeff ? a.coeff[base + t] : 1.0) * adet;
      [[maybe_unused]] double uu[NP];
      if constexpr (MODE == CELL_OPERATOR)
      {
#pragma unroll
        for (int i = 0; i < NP; ++i)
        {
          const double v = a.u[idx[i]];
          uu[i] = (a.only_fixed && !a.fixed[idx[i]]) ? 0.0 : v;
        }
      }
#pragma unroll
      for (int i = 0; i < NP; ++i)
      {
        double tm[3];
#pragma unroll
        for (int m = 0; m < 3; ++m)
        {
          const double* row = sT + (m * NP + i) * NP;
          if constexpr (MODE == CELL_DIAGONAL)
            tm[m] = row[i];
          else
          {
            double s = row[0] * uu[0];
#pragma unroll
            for (int j = 1; j < NP; ++j)
              s = s + row[j] * uu[j];
            tm[m] = s;
          }
        }
        sbuf[t * S + i] = w * ((C00 * tm[0] + C01 * tm[1]) + C11 * tm[2]);
      }
    }
  }
  __syncthreads();
  double* o = a.yloc + base * NP;
  for (int e = t; e < nloc * NP; e += PS_THREADS)
    o[e] = sbuf[(e / NP) * S + (e % NP)];
}

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

enum GatherDot
{
  DOT_NONE = 0,
  DOT_W_Y = 1, // sum_d w[d] y[d]
  DOT_R_R = 2  // sum_d r[d]^2
};

struct GatherArgs
{
  SpaceArgs s;
  const double* yloc;
  const uint8_t* fixed; // nullptr: the raw operator
  const double* add;    // nullptr or b_extra
  const double* b;      // with r: r = b - sum (0 on fixed rows)
  const double* w;      // DOT_W_Y
  double *y, *r;        // each nullptr or [ndofs]
  double* part;         // [gridDim.x] block partials of the inner product
  int32_t dot;
  const PcgState* st;
};

__global__ void __launch_bounds__(PS_THREADS) k_primal_gather(const GatherArgs a)
{
#pragma clang fp contract(off)
  __shared__ double sh[1][PS_THREADS];
  if (a.st && a.st->done)
    return;
  const SpaceArgs& s = a.s;
  const int t = threadIdx.x;
  const int64_t nshared = (int64_t)s.nnodes + (int64_t)s.nfacets * s.ne;
  double acc = 0.0;
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + t; d < s.ndofs; d += (int64_t)gridDim.x * PS_THREADS)
  {
    double v;
    if (d < nshared)
    {
      int64_t beg;
      int cnt;
      slot_range(s, d, beg, cnt);
      v = cnt > 0 ? a.yloc[s.slots[beg]] : 0.0;
      for (int k = 1; k < cnt; ++k)
        v = v + a.yloc[s.slots[beg + k]];
    }
    else
    {
      const int64_t q = d - nshared, c = q / s.ni;
      v = a.yloc[c * s.nd + 3 + 3 * s.ne + (q - c * s.ni)];
    }
    if (a.add)
      v = v + a.add[d];
    const bool fx = a.fixed && a.fixed[d];
    const double yv = fx ? 0.0 : v;
    if (a.y)
      a.y[d] = yv;
    double rv = 0.0;
    if (a.r)
    {
      rv = fx ? 0.0 : a.b[d] - v;
      a.r[d] = rv;
    }
    if (a.dot == DOT_W_Y)
      acc = acc + a.w[d] * yv;
    else if (a.dot == DOT_R_R)
      acc = acc + rv * rv;
  }
  if (a.dot == DOT_NONE)
    return;
  sh[0][t] = acc;
  __syncthreads();
  EQLB_BLOCK_TREE_SUM(sh, t, 1, PS_THREADS)
  if (t == 0)
    a.part[blockIdx.x] = sh[0][0];
}

// the mask of the listed facets; ids outside the mesh are skipped and counted (status[0]), valid ones counted (status[1])
__global__ void __launch_bounds__(PS_THREADS)
k_primal_mask(int32_t nlist, const int32_t* __restrict__ facets, int32_t nnodes, int32_t nfacets, int32_t ne,
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
  atomicAdd(status + 1, 1);
  fixed[facet_nodes[2 * (int64_t)f]] = 1;
  fixed[facet_nodes[2 * (int64_t)f + 1]] = 1;
  for (int j = 0; j < ne; ++j)
    fixed[(int64_t)nnodes + (int64_t)f * ne + j] = 1;
}

// ---- vector kernels of the iteration (grid-stride, block partials in a fixed order) -------------------------------
// z = r / diag on the free rows (0 on the fixed ones); partials of r.r and r.z: part[0][block], part[1][block]
__global__ void __launch_bounds__(PS_THREADS)
k_pcg_precond(int64_t n, const double* __restrict__ r, const double* __restrict__ diag,
              const uint8_t* __restrict__ fixed, double* __restrict__ z, double* __restrict__ part)
{
#pragma clang fp contract(off)
  __shared__ double sh[2][PS_THREADS];
  const int t = threadIdx.x, G = gridDim.x;
  double a0 = 0.0, a1 = 0.0;
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + t; d < n; d += (int64_t)G * PS_THREADS)
  {
    const double rv = r[d], zv = fixed[d] ? 0.0 : rv / diag[d];
    z[d] = zv;
    a0 = a0 + rv * rv;
    a1 = a1 + rv * zv;
  }
  sh[0][t] = a0;
  sh[1][t] = a1;
  __syncthreads();
  EQLB_BLOCK_TREE_SUM(sh, t, 2, PS_THREADS)
  if (t < 2)
    part[(int64_t)t * G + blockIdx.x] = sh[t][0];
}

// u += alpha p, r -= alpha q, z = r / diag on the free rows; the fixed rows are not touched; partials as k_pcg_precond
__global__ void __launch_bounds__(PS_THREADS)
k_pcg_update(int64_t n, const PcgState* __restrict__ st, const double* __restrict__ p, const double* __restrict__ q,
             const double* __restrict__ diag, const uint8_t* __restrict__ fixed, double* __restrict__ u,
             double* __restrict__ r, double* __restrict__ z, double* __restrict__ part)
{
#pragma clang fp contract(off)
  __shared__ double sh[2][PS_THREADS];
  if (st->done)
    return;
  const int t = threadIdx.x, G = gridDim.x;
  const double alpha = st->alpha;
  double a0 = 0.0, a1 = 0.0;
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + t; d < n; d += (int64_t)G * PS_THREADS)
  {
    if (fixed[d])
      continue; // (r and z are 0 there since the start)
    u[d] = u[d] + alpha * p[d];
    const double rv = r[d] - alpha * q[d], zv = rv / diag[d];
    r[d] = rv;
    z[d] = zv;
    a0 = a0 + rv * rv;
    a1 = a1 + rv * zv;
  }
  sh[0][t] = a0;
  sh[1][t] = a1;
  __syncthreads();
  EQLB_BLOCK_TREE_SUM(sh, t, 2, PS_THREADS)
  if (t < 2)
    part[(int64_t)t * G + blockIdx.x] = sh[t][0];
}

// p = z + beta p (first: p = z)
__global__ void __launch_bounds__(PS_THREADS)
k_pcg_direction(int64_t n, const PcgState* __restrict__ st, int first, const double* __restrict__ z,
                double* __restrict__ p)
{
#pragma clang fp contract(off)
  if (st->done)
    return;
  const double beta = first ? 0.0 : st->beta;
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x; d < n; d += (int64_t)gridDim.x * PS_THREADS)
    p[d] = first ? z[d] : z[d] + beta * p[d];
}

// u = u^: the free rows set to 0 (nothing to solve)
__global__ void __launch_bounds__(PS_THREADS)
k_pcg_clear_free(int64_t n, const uint8_t* __restrict__ fixed, double* __restrict__ u)
{
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x; d < n; d += (int64_t)gridDim.x * PS_THREADS)
    if (!fixed[d])
      u[d] = 0.0;
}

enum ScalarStep
{
  STEP_NORM = 0,    // out[0] = sqrt(channel 0)
  STEP_NB = 1,      // nb = sqrt(channel 0), tol = max(rtol nb, atol)
  STEP_START = 2,   // rr, rho from the start residual; done if it is within tol already
  STEP_ALPHA = 3,   // pq = channel 0: breakdown unless > 0, else alpha = rho / pq
  STEP_BETA = 4,    // rr, rho_new: one more iteration done; done if sqrt(rr) <= tol, else beta, rho
  STEP_TRUE = 5,    // rtrue = sqrt(channel 0); converged if <= tol
  STEP_REPLACE = 6  // after the true residual replaced r: beta = rho_new / rho, rho = rho_new, the iteration goes on
};

// one block: the channels' totals over the G block partials by the same tree, then thread 0 moves the state
__global__ void __launch_bounds__(PS_THREADS)
k_pcg_scalar(int step, int G, const double* __restrict__ part, PcgState* __restrict__ st, double rtol, double atol,
             double* __restrict__ out)
{
  __shared__ double sh[2][PS_THREADS];
  const int t = threadIdx.x;
  const bool two = step == STEP_START || step == STEP_BETA || step == STEP_REPLACE;
  if (st && st->done && step != STEP_TRUE && step != STEP_NORM && step != STEP_REPLACE)
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
      st->done = 1;
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
      st->done = 1; // (rho stays that of the last direction: STEP_REPLACE needs it if the true residual is above tol)
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
}

// ---- host side ------------------------------------------------------------------------------------------------
template <int P, int MODE>
hipError_t launch_cell_d(int d, const CellArgs& a, hipStream_t stream)
{
  const dim3 grid(grid_of(a.ncells, PS_THREADS)), block(PS_THREADS);
  if constexpr (MODE != CELL_LOAD)
    hipLaunchKernelGGL((k_primal_cell<P, MODE, 0>), grid, block, 0, stream, a);
  else
    switch (d)
    {
    case 0:
      hipLaunchKernelGGL((k_primal_cell<P, MODE, 0>), grid, block, 0, stream, a);
      break;
    case 1:
      hipLaunchKernelGGL((k_primal_cell<P, MODE, 1>), grid, block, 0, stream, a);
      break;
    case 2:
      hipLaunchKernelGGL((k_primal_cell<P, MODE, 2>), grid, block, 0, stream, a);
      break;
    default:
      hipLaunchKernelGGL((k_primal_cell<P, MODE, 3>), grid, block, 0, stream, a);
    }
  return hipGetLastError();
}

template <int MODE>
hipError_t launch_cell(int p, int d, const CellArgs& a, hipStream_t stream)
{
  switch (p)
  {
  case 1:
    return launch_cell_d<1, MODE>(d, a, stream);
  case 2:
    return launch_cell_d<2, MODE>(d, a, stream);
  case 3:
    return launch_cell_d<3, MODE>(d, a, stream);
  default:
    return launch_cell_d<4, MODE>(d, a, stream);
  }
}
} // namespace
} // namespace eqlb

// the handle behind eqlb_primal_t: everything is carved out of one allocation at create
struct eqlb_primal
{
  eqlb_mesh* mesh = nullptr;
  int p = 0, nd = 0;
  int64_t ndofs = 0;
  bool has_coeff = false;
  eqlb::SpaceArgs space{};
  eqlb::DevCarve mem;
  eqlb::DevPiece<int32_t> cell_dofs, slots, status; // status: skipped facet ids, listed valid ones, unmatched slots
  eqlb::DevPiece<double> coeff, yloc, diag, r, z, d, q, part;
  eqlb::DevPiece<uint8_t> fixed;
  eqlb::DevPiece<eqlb::PcgState> st;
};

namespace eqlb
{
namespace
{
CellArgs cell_args(const eqlb_primal& h, const double* u, bool only_fixed, const PcgState* st)
{
  CellArgs a{};
  a.ncells = h.space.ncells;
  a.cell_dofs = h.cell_dofs;
  a.cellJ = h.mesh->m.cellJ;
  a.coeff = h.has_coeff ? h.coeff.get() : nullptr;
  a.u = u;
  a.fixed = h.fixed;
  a.only_fixed = only_fixed ? 1 : 0;
  a.yloc = h.yloc;
  a.st = st;
  return a;
}

GatherArgs gather_args(const eqlb_primal& h, bool masked, const PcgState* st)
{
  GatherArgs g{};
  g.s = h.space;
  g.yloc = h.yloc;
  g.fixed = masked ? h.fixed.get() : nullptr;
  g.part = h.part;
  g.st = st;
  return g;
}

hipError_t launch_gather(const eqlb_primal& h, const GatherArgs& g, hipStream_t stream)
{
  hipLaunchKernelGGL(k_primal_gather, dim3(stream_blocks(h.ndofs)), dim3(PS_THREADS), 0, stream, g);
  return hipGetLastError();
}

hipError_t launch_scalar(const eqlb_primal& h, int step, double rtol, double atol, double* out, hipStream_t stream)
{
  hipLaunchKernelGGL(k_pcg_scalar, dim3(1), dim3(PS_THREADS), 0, stream, step, stream_blocks(h.ndofs), h.part.get(),
                     h.st.get(), rtol, atol, out);
  return hipGetLastError();
}

// y = A u (masked or raw); all pointers DEVICE
hipError_t enqueue_apply(const eqlb_primal& h, const double* u, double* y, bool masked, hipStream_t stream)
{
  hipError_t e = launch_cell<CELL_OPERATOR>(h.p, 0, cell_args(h, u, false, nullptr), stream);
  if (e != hipSuccess)
    return e;
  GatherArgs g = gather_args(h, masked, nullptr);
  g.y = y;
  return launch_gather(h, g, stream);
}

hipError_t enqueue_diagonal(const eqlb_primal& h, double* out, hipStream_t stream)
{
  hipError_t e = launch_cell<CELL_DIAGONAL>(h.p, 0, cell_args(h, nullptr, false, nullptr), stream);
  if (e != hipSuccess)
    return e;
  GatherArgs g = gather_args(h, false, nullptr);
  g.y = out;
  return launch_gather(h, g, stream);
}

// r = b - A u (0 on the fixed rows), u^ instead of u with only_fixed; the block partials of r.r are left in h.part
hipError_t enqueue_residual(const eqlb_primal& h, const double* b, const double* u, double* r, bool only_fixed,
                            hipStream_t stream)
{
  hipError_t e = launch_cell<CELL_OPERATOR>(h.p, 0, cell_args(h, u, only_fixed, nullptr), stream);
  if (e != hipSuccess)
    return e;
  GatherArgs g = gather_args(h, true, nullptr);
  g.b = b;
  g.r = r;
  g.dot = DOT_R_R;
  return launch_gather(h, g, stream);
}

int check_handle(const char* who, const eqlb_primal* h)
{
  if (!h)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null handle", who);
  return EQLB_OK;
}
} // namespace
} // namespace eqlb

extern "C" {

int eqlb_get_stiffness_table(int32_t p, double* out, int32_t capacity)
{
  using namespace eqlb;
  if (p < 1 || p > PS_PMAX || !out)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_get_stiffness_table: p = %d outside 1 ... 4, or null output", (int)p);
  const int n = 3 * nd_of(p) * nd_of(p);
  if (capacity < n)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_get_stiffness_table: capacity too small");
  const double* t = p == 1 ? eqlb_tables::Stiff<1>::ST
                           : p == 2 ? eqlb_tables::Stiff<2>::ST
                                    : p == 3 ? eqlb_tables::Stiff<3>::ST : eqlb_tables::Stiff<4>::ST;
  for (int i = 0; i < n; ++i)
    out[i] = t[i];
  return n;
}

int eqlb_get_load_table(int32_t p, int32_t d, double* out, int32_t capacity)
{
  using namespace eqlb;
  if (p < 1 || p > PS_PMAX || d < 0 || d > PS_DMAX || !out)
    return fail(EQLB_ERR_INVALID_ARGUMENT,
                "eqlb_get_load_table: degrees p = %d, degree_dg = %d outside 1 ... 4, 0 ... 3, or null output", (int)p,
                (int)d);
  const int n = nd_of(p) * nd_of(d);
  if (capacity < n)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_get_load_table: capacity too small");
  const double* t = nullptr;
#define EQLB_LOAD_ROW(PP)                                                                                              \
  case PP:                                                                                                             \
    t = d == 0 ? eqlb_tables::Load<PP, 0>::LD                                                                          \
               : d == 1 ? eqlb_tables::Load<PP, 1>::LD                                                                 \
                        : d == 2 ? eqlb_tables::Load<PP, 2>::LD : eqlb_tables::Load<PP, 3>::LD;                        \
    break;
  switch (p)
  {
    EQLB_LOAD_ROW(1)
    EQLB_LOAD_ROW(2)
    EQLB_LOAD_ROW(3)
    EQLB_LOAD_ROW(4)
  }
#undef EQLB_LOAD_ROW
  for (int i = 0; i < n; ++i)
    out[i] = t[i];
  return n;
}

int eqlb_primal_create(eqlb_mesh_t* mesh, int32_t p, const double* cell_coeff, int32_t memspace, void* stream_,
                       eqlb_primal_t** handle)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_primal_create";
  if (p < 1 || p > PS_PMAX)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: p = %d outside 1 ... 4", who, (int)p);
  if (!mesh || !handle)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  EQLB_TRY(check_memspace(who, memspace));
  const DeviceMesh& m = mesh->m;
  const int ne = p - 1, ni = (p - 1) * (p - 2) / 2, nd = nd_of(p);
  const int64_t ndofs = (int64_t)m.nnodes + (int64_t)m.nfacets * ne + (int64_t)m.ncells * ni;
  if (ndofs > INT32_MAX || (int64_t)m.ncells * nd > INT32_MAX || m.ncells < 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: %lld DOFs, %lld cell entries do not fit 32 bits", who, (long long)ndofs,
                (long long)m.ncells * nd);
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  // a handle of eqlb_mesh_create keeps node -> cell on the host until somebody needs it on the device
  const int32_t* node_cells = nullptr;
  if (mesh_node_cells(mesh, &node_cells))
    return EQLB_ERR_DEVICE;
  std::unique_ptr<eqlb_primal> h(new eqlb_primal);
  h->mesh = mesh;
  h->p = p;
  h->nd = nd;
  h->ndofs = ndofs;
  h->has_coeff = cell_coeff != nullptr;
  const size_t nc = (size_t)m.ncells, nslots = 3 * nc * (size_t)(1 + ne);
  h->cell_dofs = h->mem.piece<int32_t>(nc * nd);
  h->slots = h->mem.piece<int32_t>(nslots);
  h->status = h->mem.piece<int32_t>(4);
  h->coeff = h->mem.piece<double>(nc);
  h->yloc = h->mem.piece<double>(nc * nd);
  h->diag = h->mem.piece<double>((size_t)ndofs);
  h->r = h->mem.piece<double>((size_t)ndofs);
  h->z = h->mem.piece<double>((size_t)ndofs);
  h->d = h->mem.piece<double>((size_t)ndofs);
  h->q = h->mem.piece<double>((size_t)ndofs);
  h->part = h->mem.piece<double>(2 * (size_t)PS_MAXBLOCKS);
  h->fixed = h->mem.piece<uint8_t>((size_t)ndofs);
  h->st = h->mem.piece<PcgState>(1);
  HIP_TRY(h->mem.alloc());
  SpaceArgs& s = h->space;
  s.ndofs = ndofs;
  s.nnodes = m.nnodes;
  s.nfacets = m.nfacets;
  s.ncells = m.ncells;
  s.ne = ne;
  s.ni = ni > 0 ? ni : 1;
  s.nd = nd;
  s.nco = m.node_cells_off;
  s.fco = m.facet_cells_off;
  s.slots = h->slots;
  HIP_TRY(hipMemsetAsync(h->status, 0, 4 * sizeof(int32_t), stream));
  HIP_TRY(hipMemsetAsync(h->fixed, 0, (size_t)ndofs, stream));
  if (cell_coeff)
    HIP_TRY(hipMemcpyAsync(h->coeff, cell_coeff, nc * sizeof(double),
                           memspace == EQLB_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, stream));
  // the dofmap, by the kernel behind eqlb_mesh_lagrange_dofmap (device memory space: one launch, nothing waits)
  EQLB_TRY(eqlb_mesh_lagrange_dofmap(mesh, p, h->cell_dofs.get(), nullptr, EQLB_MEM_DEVICE, stream_));
  const int64_t nshared = (int64_t)m.nnodes + (int64_t)m.nfacets * ne;
  hipLaunchKernelGGL(k_primal_slots, dim3(grid_of(nshared, PS_THREADS)), dim3(PS_THREADS), 0, stream, s, node_cells,
                     m.facet_cells, h->cell_dofs.get(), h->slots.get(), h->status.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(enqueue_diagonal(*h, h->diag, stream));
  if (memspace == EQLB_MEM_HOST)
    HIP_TRY(hipStreamSynchronize(stream)); // (the caller's coefficient array has been read)
  *handle = h.release();
  return EQLB_OK;
}
EQLB_CATCH_ALL

void eqlb_primal_destroy(eqlb_primal_t* handle) { delete handle; }

int eqlb_primal_ndofs(const eqlb_primal_t* handle, int64_t* ndofs)
{
  using namespace eqlb;
  if (!handle || !ndofs)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_primal_ndofs: null argument");
  *ndofs = handle->ndofs;
  return EQLB_OK;
}

int eqlb_primal_set_dirichlet(eqlb_primal_t* h, int32_t nlist, const int32_t* facets, int32_t memspace, void* stream_)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_primal_set_dirichlet";
  if (nlist < 0 || (nlist > 0 && !facets))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: nlist = %d, or a null list", who, (int)nlist);
  EQLB_TRY(check_handle(who, h));
  EQLB_TRY(check_memspace(who, memspace));
  const DeviceMesh& m = h->mesh->m;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool host = memspace == EQLB_MEM_HOST;
  if (host)
    for (int32_t i = 0; i < nlist; ++i)
      if (facets[i] < 0 || facets[i] >= m.nfacets)
        return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: facets[%d] = %d is no facet of the mesh (%d facets)", who, (int)i,
                    (int)facets[i], (int)m.nfacets);
  HostCall s; // (a device-memory call stages nothing: no allocation, no copy and no wait)
  const auto d_f = s.in(host ? facets : nullptr, (size_t)nlist);
  if (host && nlist > 0)
    HIP_TRY(s.upload(stream));
  s.note(hipMemsetAsync(h->fixed, 0, (size_t)h->ndofs, stream));
  s.note(hipMemsetAsync(h->status, 0, 2 * sizeof(int32_t), stream));
  if (nlist > 0)
  {
    hipLaunchKernelGGL(k_primal_mask, dim3(grid_of(nlist, PS_THREADS)), dim3(PS_THREADS), 0, stream, nlist,
                       host ? d_f.get() : facets, m.nnodes, m.nfacets, h->space.ne, m.facet_nodes, h->fixed.get(),
                       h->status.get());
    s.note(hipGetLastError());
  }
  HIP_TRY(s.finish(stream));
  return EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_primal_load(eqlb_primal_t* h, int32_t degree_dg, const double* rhs_dg, const double* b_extra, double* b,
                     int32_t memspace, void* stream_)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_primal_load";
  if (degree_dg < 0 || degree_dg > PS_DMAX)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: degree_dg = %d outside 0 ... 3", who, (int)degree_dg);
  EQLB_TRY(check_handle(who, h));
  if (!rhs_dg || !b)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  EQLB_TRY(check_memspace(who, memspace));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool host = memspace == EQLB_MEM_HOST;
  const size_t nf = (size_t)h->space.ncells * nd_of(degree_dg), n = (size_t)h->ndofs;
  HostCall s;
  const auto d_f = s.in(host ? rhs_dg : nullptr, nf), d_e = s.in(host ? b_extra : nullptr, n);
  const auto d_b = s.out(host ? b : nullptr, n);
  if (host)
    HIP_TRY(s.upload(stream));
  s.note(launch_cell<CELL_LOAD>(h->p, degree_dg, cell_args(*h, host ? d_f.get() : rhs_dg, false, nullptr), stream));
  GatherArgs g = gather_args(*h, false, nullptr);
  g.add = host ? d_e.get() : b_extra;
  g.y = host ? d_b.get() : b;
  s.note(launch_gather(*h, g, stream));
  HIP_TRY(s.finish(stream));
  return EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_primal_apply(eqlb_primal_t* h, const double* u, double* y, int32_t masked, int32_t memspace, void* stream_)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_primal_apply";
  EQLB_TRY(check_handle(who, h));
  if (!u || !y)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  EQLB_TRY(check_memspace(who, memspace));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool host = memspace == EQLB_MEM_HOST;
  const size_t n = (size_t)h->ndofs;
  HostCall s;
  const auto d_u = s.in(host ? u : nullptr, n);
  const auto d_y = s.out(host ? y : nullptr, n);
  if (host)
    HIP_TRY(s.upload(stream));
  s.note(enqueue_apply(*h, host ? d_u.get() : u, host ? d_y.get() : y, masked != 0, stream));
  HIP_TRY(s.finish(stream));
  return EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_primal_diagonal(eqlb_primal_t* h, double* out, int32_t memspace, void* stream_)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_primal_diagonal";
  EQLB_TRY(check_handle(who, h));
  if (!out)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  EQLB_TRY(check_memspace(who, memspace));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool host = memspace == EQLB_MEM_HOST;
  HostCall s;
  const auto d_o = s.out(host ? out : nullptr, (size_t)h->ndofs);
  if (host)
    HIP_TRY(s.upload(stream));
  s.note(enqueue_diagonal(*h, host ? d_o.get() : out, stream));
  HIP_TRY(s.finish(stream));
  return EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_primal_residual(eqlb_primal_t* h, const double* b, const double* u, double* r, double* norms,
                         int32_t memspace, void* stream_)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_primal_residual";
  EQLB_TRY(check_handle(who, h));
  if (!b || !u || !r)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  EQLB_TRY(check_memspace(who, memspace));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool host = memspace == EQLB_MEM_HOST;
  const size_t n = (size_t)h->ndofs;
  HostCall s;
  const auto d_b = s.in(host ? b : nullptr, n), d_u = s.in(host ? u : nullptr, n);
  const auto d_r = s.out(host ? r : nullptr, n);
  const auto d_n = s.out(host ? norms : nullptr, 2);
  if (host)
    HIP_TRY(s.upload(stream));
  const double *pb = host ? d_b.get() : b, *pu = host ? d_u.get() : u;
  double* pn = host ? d_n.get() : norms;
  if (pn)
  {
    // the reference norm first, into the work vector q: the residual proper then leaves r as the caller sees it
    s.note(enqueue_residual(*h, pb, pu, h->q, true, stream));
    s.note(launch_scalar(*h, STEP_NORM, 0.0, 0.0, pn + 1, stream));
  }
  s.note(enqueue_residual(*h, pb, pu, host ? d_r.get() : r, false, stream));
  if (pn)
    s.note(launch_scalar(*h, STEP_NORM, 0.0, 0.0, pn, stream));
  HIP_TRY(s.finish(stream));
  return EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_primal_solve(eqlb_primal_t* h, const double* b, double* u, double rtol, double atol, int32_t maxit,
                      double* info, int32_t memspace, void* stream_)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_primal_solve";
  if (maxit < 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: maxit = %d (at least 1)", who, (int)maxit);
  if (!(rtol >= 0.0) || !(atol >= 0.0))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: rtol = %g, atol = %g negative or NaN", who, rtol, atol);
  EQLB_TRY(check_handle(who, h));
  if (!b || !u || !info)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  EQLB_TRY(check_memspace(who, memspace));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  // the status word of the mask: the call waits by nature, and nothing is launched for a singular problem
  int32_t status[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(status, h->status.get(), sizeof(status), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  if (status[1] < 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: singular: no Dirichlet DOF (eqlb_primal_set_dirichlet first)", who);
  const bool host = memspace == EQLB_MEM_HOST;
  const size_t n = (size_t)h->ndofs;
  HostCall s;
  const auto d_b = s.in(host ? b : nullptr, n);
  const auto d_u = s.in(host ? static_cast<const double*>(u) : nullptr, n);
  if (host)
    HIP_TRY(s.upload(stream));
  const double* pb = host ? d_b.get() : b;
  double* pu = host ? d_u.get() : u;
  PcgState* st = h->st;
  const int G = stream_blocks(h->ndofs);
  const dim3 grid(G), block(PS_THREADS);
  const int64_t nn = h->ndofs;
  PcgState hs{};
  auto read_state = [&]() -> hipError_t {
    hipError_t e = hipMemcpyAsync(&hs, st, sizeof(PcgState), hipMemcpyDeviceToHost, stream);
    return e != hipSuccess ? e : hipStreamSynchronize(stream);
  };
  // the true residual of the current u into q, its norm into the state
  auto true_residual = [&]() {
    s.note(enqueue_residual(*h, pb, pu, h->q, false, stream));
    s.note(launch_scalar(*h, STEP_TRUE, rtol, atol, nullptr, stream));
  };
  s.note(hipMemsetAsync(st, 0, sizeof(PcgState), stream));
  // nb and tol from u^
  s.note(enqueue_residual(*h, pb, pu, h->q, true, stream));
  s.note(launch_scalar(*h, STEP_NB, rtol, atol, nullptr, stream));
  // the start: r = b - A u, z = r / diag, rho, p = z
  s.note(enqueue_residual(*h, pb, pu, h->r, false, stream));
  hipLaunchKernelGGL(k_pcg_precond, grid, block, 0, stream, nn, h->r.get(), h->diag.get(), h->fixed.get(), h->z.get(),
                     h->part.get());
  s.note(launch_scalar(*h, STEP_START, rtol, atol, nullptr, stream));
  hipLaunchKernelGGL(k_pcg_direction, grid, block, 0, stream, nn, st, 1, h->z.get(), h->d.get());
  s.note(hipGetLastError());
  s.note(read_state());
  bool have_true = false; // q holds the true residual of the current u and the state its norm
  if (s.finish(stream) == hipSuccess && hs.tol == 0.0 && hs.nb == 0.0)
  {
    // nothing to solve: u^ is the solution (the free rows of u are set to 0 by the start residual's mask)
    hipLaunchKernelGGL(k_pcg_clear_free, grid, block, 0, stream, nn, h->fixed.get(), pu);
    s.note(hipGetLastError());
    hs.converged = 1;
    hs.rtrue = 0.0;
    have_true = true;
  }
  else
  {
    while (s.finish(stream) == hipSuccess && !hs.breakdown && !hs.converged)
    {
      if (hs.done)
      {
        // the recurrence residual reached tol: the true one decides
        true_residual();
        s.note(read_state());
        have_true = true;
        if (hs.converged || hs.iters >= maxit)
          break;
        s.note(hipMemcpyAsync(h->r.get(), h->q.get(), n * sizeof(double), hipMemcpyDeviceToDevice, stream));
        hipLaunchKernelGGL(k_pcg_precond, grid, block, 0, stream, nn, h->r.get(), h->diag.get(), h->fixed.get(),
                           h->z.get(), h->part.get());
        s.note(launch_scalar(*h, STEP_REPLACE, rtol, atol, nullptr, stream));
        hipLaunchKernelGGL(k_pcg_direction, grid, block, 0, stream, nn, st, 0, h->z.get(), h->d.get());
        s.note(hipGetLastError());
        have_true = false;
      }
      if (hs.iters >= maxit)
        break;
      const int batch = (maxit - hs.iters < PRIMAL_CHECK_EVERY) ? maxit - hs.iters : PRIMAL_CHECK_EVERY;
      for (int it = 0; it < batch; ++it)
      {
        s.note(launch_cell<CELL_OPERATOR>(h->p, 0, cell_args(*h, h->d, false, st), stream));
        GatherArgs g = gather_args(*h, true, st);
        g.y = h->q;
        g.w = h->d;
        g.dot = DOT_W_Y;
        s.note(launch_gather(*h, g, stream));
        s.note(launch_scalar(*h, STEP_ALPHA, rtol, atol, nullptr, stream));
        hipLaunchKernelGGL(k_pcg_update, grid, block, 0, stream, nn, st, h->d.get(), h->q.get(), h->diag.get(),
                           h->fixed.get(), pu, h->r.get(), h->z.get(), h->part.get());
        s.note(launch_scalar(*h, STEP_BETA, rtol, atol, nullptr, stream));
        hipLaunchKernelGGL(k_pcg_direction, grid, block, 0, stream, nn, st, 0, h->z.get(), h->d.get());
        s.note(hipGetLastError());
      }
      have_true = false;
      s.note(read_state());
    }
  }
  if (!have_true)
  {
    true_residual();
    const int conv = hs.converged;
    s.note(read_state());
    hs.converged = conv; // (a run that ended at maxit or broke down is not converged, whatever its last residual)
  }
  if (host)
    s.out_prefix(u, d_u, n);
  HIP_TRY(s.finish(stream));
  info[0] = (double)hs.iters;
  info[1] = (double)hs.converged;
  info[2] = hs.nb;
  info[3] = hs.rtrue;
  info[4] = (double)hs.replacements;
  info[5] = (double)hs.breakdown;
  info[6] = hs.tol;
  info[7] = (double)status[0];
  return EQLB_OK;
}
EQLB_CATCH_ALL

} // extern "C"
