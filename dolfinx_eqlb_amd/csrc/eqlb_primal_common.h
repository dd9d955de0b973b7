// What the P_p Poisson solve (eqlb_primal_solve.hip) and the P_p^2 elasticity solve (eqlb_primal_elasticity.hip) share:
// the sum pass of the store-and-sum operator, the vector kernels and the scalar kernel of the Jacobi-preconditioned CG,
// and the host loop that drives them.  Everything lies in an unnamed namespace: each unit gets its own copy, under the
// names the kernels had while they lived in eqlb_primal_solve.hip.  The hierarchy unit (eqlb_multilevel.hip) takes the
// state, the scalar and direction kernels and the host loop from here and brings its own preconditioner steps.
//  k_primal_slots    builds the slot lists of the sum pass once at create (scalar numbering: both problems use it)
//  k_primal_gather<BS>  one thread per (DOF, component): BS values per y_loc entry, the vectors blocked
//                    x[BS * dof + r].  BS = 1 is the kernel of the Poisson unit, instruction for instruction
//  k_pcg_*           work on any length n with a byte mask [n]: n = ndofs or 2 ndofs
//  pcg_solve         the host side of the iteration on a PcgWork; the preconditioner enters through its `steps`
//                    (JacobiSteps here; the hierarchy unit eqlb_multilevel.hip brings its own)
#pragma once

#include "eqlb_device_common.h"
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

// scalars of the iteration, in device memory
struct PcgState
{
  double rho, pq, alpha, beta, rr, nb, tol, rtrue;
  int32_t iters, done, breakdown, converged, replacements, pad;
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

// the sum pass with BS components per DOF: e = BS d + r runs over the blocked vectors, y_loc holds BS values per
// (cell, local index), the component fastest.  BS = 1 is the sum pass of the Poisson problem as it was
template <int BS>
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
  for (int64_t e = (int64_t)blockIdx.x * PS_THREADS + t; e < s.ndofs * BS; e += (int64_t)gridDim.x * PS_THREADS)
  {
    const int64_t d = e / BS;
    const int r = (int)(e - d * BS);
    double v;
    if (d < nshared)
    {
      int64_t beg;
      int cnt;
      slot_range(s, d, beg, cnt);
      v = cnt > 0 ? a.yloc[(int64_t)s.slots[beg] * BS + r] : 0.0;
      for (int k = 1; k < cnt; ++k)
        v = v + a.yloc[(int64_t)s.slots[beg + k] * BS + r];
    }
    else
    {
      const int64_t q = d - nshared, c = q / s.ni;
      v = a.yloc[(c * s.nd + 3 + 3 * s.ne + (q - c * s.ni)) * BS + r];
    }
    if (a.add)
      v = v + a.add[e];
    const bool fx = a.fixed && a.fixed[e];
    const double yv = fx ? 0.0 : v;
    if (a.y)
      a.y[e] = yv;
    double rv = 0.0;
    if (a.r)
    {
      rv = fx ? 0.0 : a.b[e] - v;
      a.r[e] = rv;
    }
    if (a.dot == DOT_W_Y)
      acc = acc + a.w[e] * yv;
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

// ---- host side of the iteration ------------------------------------------------------------------------------------
// the vectors of one handle: n rows (the blocked length), all in device memory
struct PcgWork
{
  int64_t n;
  const double* diag;
  const uint8_t* fixed;
  double *r, *z, *d, *q, *part;
  PcgState* st;
};

inline hipError_t launch_scalar(const PcgWork& w, int step, double rtol, double atol, double* out, hipStream_t stream)
{
  hipLaunchKernelGGL(k_pcg_scalar, dim3(1), dim3(PS_THREADS), 0, stream, step, stream_blocks(w.n), w.part, w.st, rtol,
                     atol, out);
  return hipGetLastError();
}

// The two places where the preconditioner enters the iteration, for z = r / diag: both kernels fuse it
struct JacobiSteps
{
  static constexpr int check_every = PRIMAL_CHECK_EVERY; // iterations between two reads of the state by the host
  const PcgWork& w;
  hipStream_t stream;
  // z from the r of the start or of a replacement, the partials of r.r and r.z, the scalar step (STEP_START / _REPLACE)
  hipError_t restart(int step, double rtol, double atol) const
  {
    hipLaunchKernelGGL(k_pcg_precond, dim3(stream_blocks(w.n)), dim3(PS_THREADS), 0, stream, w.n, w.r, w.diag, w.fixed,
                       w.z, w.part);
    return launch_scalar(w, step, rtol, atol, nullptr, stream);
  }
  // u += alpha d, r -= alpha q, z from the new r, the partials of r.r and r.z, STEP_BETA
  hipError_t advance(double* pu, double rtol, double atol) const
  {
    hipLaunchKernelGGL(k_pcg_update, dim3(stream_blocks(w.n)), dim3(PS_THREADS), 0, stream, w.n, w.st, w.d, w.q, w.diag,
                       w.fixed, pu, w.r, w.z, w.part);
    return launch_scalar(w, STEP_BETA, rtol, atol, nullptr, stream);
  }
};

// The preconditioned CG of eqlb_primal_solve / eqlb_elasticity_solve / eqlb_hierarchy_solve behind their argument checks.
//   residual(b, u, r, only_fixed)  enqueues r = b - A u (0 on the fixed rows; u^ instead of u with only_fixed) and
//                                  leaves the block partials of r.r in w.part
//   product(st)                    enqueues q = A d on the free rows with the block partials of d.q in w.part
//   steps                          the preconditioner: restart(step, rtol, atol) and advance(u, rtol, atol) as JacobiSteps
// skipped: the facet ids the mask skipped (info[7]).  b, u in host memory with `host` are staged here.
template <class Residual, class Product, class Steps>
int pcg_solve(const PcgWork& w, Residual&& residual, Product&& product, const Steps& steps, const double* b, double* u,
              double rtol, double atol, int32_t maxit, double* info, int32_t skipped, bool host, hipStream_t stream)
{
  const size_t n = (size_t)w.n;
  HostCall s;
  const auto d_b = s.in(host ? b : nullptr, n);
  const auto d_u = s.in(host ? static_cast<const double*>(u) : nullptr, n);
  if (host)
    HIP_TRY(s.upload(stream));
  const double* pb = host ? d_b.get() : b;
  double* pu = host ? d_u.get() : u;
  PcgState* st = w.st;
  const int G = stream_blocks(w.n);
  const dim3 grid(G), block(PS_THREADS);
  const int64_t nn = w.n;
  PcgState hs{};
  auto read_state = [&]() -> hipError_t {
    hipError_t e = hipMemcpyAsync(&hs, st, sizeof(PcgState), hipMemcpyDeviceToHost, stream);
    return e != hipSuccess ? e : hipStreamSynchronize(stream);
  };
  // the true residual of the current u into q, its norm into the state
  auto true_residual = [&]() {
    s.note(residual(pb, pu, w.q, false));
    s.note(launch_scalar(w, STEP_TRUE, rtol, atol, nullptr, stream));
  };
  s.note(hipMemsetAsync(st, 0, sizeof(PcgState), stream));
  // nb and tol from u^
  s.note(residual(pb, pu, w.q, true));
  s.note(launch_scalar(w, STEP_NB, rtol, atol, nullptr, stream));
  // the start: r = b - A u, z from r, rho, p = z
  s.note(residual(pb, pu, w.r, false));
  s.note(steps.restart(STEP_START, rtol, atol));
  hipLaunchKernelGGL(k_pcg_direction, grid, block, 0, stream, nn, st, 1, w.z, w.d);
  s.note(hipGetLastError());
  s.note(read_state());
  bool have_true = false; // q holds the true residual of the current u and the state its norm
  if (s.finish(stream) == hipSuccess && hs.tol == 0.0 && hs.nb == 0.0)
  {
    // nothing to solve: u^ is the solution (the free rows of u are set to 0 by the start residual's mask)
    hipLaunchKernelGGL(k_pcg_clear_free, grid, block, 0, stream, nn, w.fixed, pu);
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
        s.note(hipMemcpyAsync(w.r, w.q, n * sizeof(double), hipMemcpyDeviceToDevice, stream));
        s.note(steps.restart(STEP_REPLACE, rtol, atol));
        hipLaunchKernelGGL(k_pcg_direction, grid, block, 0, stream, nn, st, 0, w.z, w.d);
        s.note(hipGetLastError());
        have_true = false;
      }
      if (hs.iters >= maxit)
        break;
      const int batch = (maxit - hs.iters < Steps::check_every) ? maxit - hs.iters : Steps::check_every;
      for (int it = 0; it < batch; ++it)
      {
        s.note(product(st));
        s.note(launch_scalar(w, STEP_ALPHA, rtol, atol, nullptr, stream));
        s.note(steps.advance(pu, rtol, atol));
        hipLaunchKernelGGL(k_pcg_direction, grid, block, 0, stream, nn, st, 0, w.z, w.d);
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
  info[7] = (double)skipped;
  return EQLB_OK;
}
} // namespace
} // namespace eqlb
