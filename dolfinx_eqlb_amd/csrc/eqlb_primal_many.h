// Several right-hand sides in one P_p Poisson solve (eqlb_primal_*_many, eqlb_hierarchy_*_many of include/eqlb.h): the
// column variants of the sum pass, of the CG kernels and of the host loop of eqlb_primal_common.h.  THE RULE: column c
// of a many-solve is the single solve of (b_c, u_c) - the same bits, the same info.  What makes it hold:
//  - one thread per DOF carries the values of that DOF in all columns: the grid is stream_blocks(ndofs), the per-thread
//    order over the DOFs and the block tree are those of the single kernels, so every inner product of a column is the
//    sum the single solve forms.  Block partials [R][2][G];
//  - every column has its own PcgState; a kernel works on the columns of its ManyCols (eqlb_internal.h) and leaves the
//    others alone, so a column freezes at its stop flag while the others go on, and waits untouched for the host;
//  - k_pcg_scalar_many runs one block per column with the body of k_pcg_scalar.
// Vectors are [R][n], one column after another (the layout eqlb_primal_flux_dg and eqlb_refine_prolong_lagrange read);
// R <= MANY_R columns per group, a larger count runs group after group.  Included by eqlb_primal_solve.hip and
// eqlb_multilevel.hip; the single-vector kernels are not touched.
#pragma once

#include "eqlb_primal_common.h"

namespace eqlb
{
namespace
{
constexpr int MANY_R = 4; // columns of one group

// bit c: column c runs in this launch
__device__ __forceinline__ uint32_t many_live(const ManyCols& c)
{
  const PcgState* st = static_cast<const PcgState*>(c.st);
  uint32_t live = 0;
#pragma unroll
  for (int k = 0; k < MANY_R; ++k)
    if (k < c.R && ((c.mask >> k) & 1u) && !(c.check && st[k].done))
      live |= 1u << k;
  return live;
}

struct ManyGatherArgs
{
  GatherArgs g;    // y, r, b, w: column 0 of [R][ndofs]; part: [R][2][G], channel 0 is written; add is not read
  ManyCols cols;
  int64_t ystride; // y_loc of column c: g.yloc + c * ystride
};

// k_primal_gather<1> on the live columns: the slot range of a DOF is found once, the sum of a column runs in the order
// of the slot list as in the single kernel
__global__ void __launch_bounds__(PS_THREADS) k_primal_gather_many(const ManyGatherArgs m)
{
#pragma clang fp contract(off)
  __shared__ double sh[MANY_R][PS_THREADS];
  const uint32_t live = many_live(m.cols);
  if (!live)
    return;
  const GatherArgs& a = m.g;
  const SpaceArgs& s = a.s;
  const int t = threadIdx.x;
  const int64_t nshared = (int64_t)s.nnodes + (int64_t)s.nfacets * s.ne;
  double acc[MANY_R] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + t; d < s.ndofs; d += (int64_t)gridDim.x * PS_THREADS)
  {
    int64_t beg = 0;
    int cnt = 0;
    if (d < nshared)
      slot_range(s, d, beg, cnt);
    else
    {
      const int64_t q = d - nshared, c = q / s.ni;
      beg = c * s.nd + 3 + 3 * s.ne + (q - c * s.ni); // (the one entry of an interior DOF)
    }
    const bool fx = a.fixed && a.fixed[d];
#pragma unroll
    for (int k = 0; k < MANY_R; ++k)
    {
      if (!((live >> k) & 1u))
        continue;
      const double* yl = a.yloc + k * m.ystride;
      double v;
      if (d < nshared)
      {
        v = cnt > 0 ? yl[s.slots[beg]] : 0.0;
        for (int j = 1; j < cnt; ++j)
          v = v + yl[s.slots[beg + j]];
      }
      else
        v = yl[beg];
      const int64_t e = k * s.ndofs + d;
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
        acc[k] = acc[k] + a.w[e] * yv;
      else if (a.dot == DOT_R_R)
        acc[k] = acc[k] + rv * rv;
    }
  }
  if (a.dot == DOT_NONE)
    return;
#pragma unroll
  for (int k = 0; k < MANY_R; ++k)
    sh[k][t] = acc[k];
  __syncthreads();
  EQLB_BLOCK_TREE_SUM(sh, t, MANY_R, PS_THREADS)
  if (t < MANY_R && ((live >> t) & 1u))
    a.part[(int64_t)(2 * t) * gridDim.x + blockIdx.x] = sh[t][0];
}

// ---- vector kernels of the iteration: the single ones with the columns of a DOF in one thread ----------------------
// channel j of column k: sh[2 k + j], part[(2 k + j) G + block]
__global__ void __launch_bounds__(PS_THREADS)
k_pcg_precond_many(int64_t n, const ManyCols cols, const double* __restrict__ r, const double* __restrict__ diag,
                   const uint8_t* __restrict__ fixed, double* __restrict__ z, double* __restrict__ part)
{
#pragma clang fp contract(off)
  __shared__ double sh[2 * MANY_R][PS_THREADS];
  const uint32_t live = many_live(cols);
  if (!live)
    return;
  const int t = threadIdx.x, G = gridDim.x;
  double a0[MANY_R] = {0.0, 0.0, 0.0, 0.0}, a1[MANY_R] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + t; d < n; d += (int64_t)G * PS_THREADS)
  {
    const bool fx = fixed[d];
    const double dg = diag[d];
#pragma unroll
    for (int k = 0; k < MANY_R; ++k)
    {
      if (!((live >> k) & 1u))
        continue;
      const double rv = r[k * n + d], zv = fx ? 0.0 : rv / dg;
      z[k * n + d] = zv;
      a0[k] = a0[k] + rv * rv;
      a1[k] = a1[k] + rv * zv;
    }
  }
#pragma unroll
  for (int k = 0; k < MANY_R; ++k)
  {
    sh[2 * k][t] = a0[k];
    sh[2 * k + 1][t] = a1[k];
  }
  __syncthreads();
  EQLB_BLOCK_TREE_SUM(sh, t, 2 * MANY_R, PS_THREADS)
  if (t < 2 * MANY_R && ((live >> (t / 2)) & 1u))
    part[(int64_t)t * G + blockIdx.x] = sh[t][0];
}

__global__ void __launch_bounds__(PS_THREADS)
k_pcg_update_many(int64_t n, const ManyCols cols, const double* __restrict__ p, const double* __restrict__ q,
                  const double* __restrict__ diag, const uint8_t* __restrict__ fixed, double* __restrict__ u,
                  double* __restrict__ r, double* __restrict__ z, double* __restrict__ part)
{
#pragma clang fp contract(off)
  __shared__ double sh[2 * MANY_R][PS_THREADS];
  const uint32_t live = many_live(cols);
  if (!live)
    return;
  const PcgState* st = static_cast<const PcgState*>(cols.st);
  const int t = threadIdx.x, G = gridDim.x;
  double alpha[MANY_R];
#pragma unroll
  for (int k = 0; k < MANY_R; ++k)
    alpha[k] = ((live >> k) & 1u) ? st[k].alpha : 0.0;
  double a0[MANY_R] = {0.0, 0.0, 0.0, 0.0}, a1[MANY_R] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + t; d < n; d += (int64_t)G * PS_THREADS)
  {
    if (fixed[d])
      continue; // (r and z are 0 there since the start)
    const double dg = diag[d];
#pragma unroll
    for (int k = 0; k < MANY_R; ++k)
    {
      if (!((live >> k) & 1u))
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
  for (int k = 0; k < MANY_R; ++k)
  {
    sh[2 * k][t] = a0[k];
    sh[2 * k + 1][t] = a1[k];
  }
  __syncthreads();
  EQLB_BLOCK_TREE_SUM(sh, t, 2 * MANY_R, PS_THREADS)
  if (t < 2 * MANY_R && ((live >> (t / 2)) & 1u))
    part[(int64_t)t * G + blockIdx.x] = sh[t][0];
}

__global__ void __launch_bounds__(PS_THREADS)
k_pcg_direction_many(int64_t n, const ManyCols cols, int first, const double* __restrict__ z, double* __restrict__ p)
{
#pragma clang fp contract(off)
  const uint32_t live = many_live(cols);
  if (!live)
    return;
  const PcgState* st = static_cast<const PcgState*>(cols.st);
  double beta[MANY_R];
#pragma unroll
  for (int k = 0; k < MANY_R; ++k)
    beta[k] = (!first && ((live >> k) & 1u)) ? st[k].beta : 0.0;
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x; d < n; d += (int64_t)gridDim.x * PS_THREADS)
  {
#pragma unroll
    for (int k = 0; k < MANY_R; ++k)
    {
      if (!((live >> k) & 1u))
        continue;
      const int64_t e = k * n + d;
      p[e] = first ? z[e] : z[e] + beta[k] * p[e];
    }
  }
}

__global__ void __launch_bounds__(PS_THREADS)
k_pcg_clear_free_many(int64_t n, const ManyCols cols, const uint8_t* __restrict__ fixed, double* __restrict__ u)
{
  const uint32_t live = many_live(cols);
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x; d < n; d += (int64_t)gridDim.x * PS_THREADS)
    if (!fixed[d])
    {
#pragma unroll
      for (int k = 0; k < MANY_R; ++k)
        if ((live >> k) & 1u)
          u[k * n + d] = 0.0;
    }
}

// k_pcg_scalar, one block per column: block k moves the state of column k from its own partials (the stop flag is
// looked at per step, as there; mask picks the columns)
__global__ void __launch_bounds__(PS_THREADS)
k_pcg_scalar_many(int step, int G, uint32_t mask, const double* __restrict__ part_, PcgState* __restrict__ st_,
                  double rtol, double atol)
{
  __shared__ double sh[2][PS_THREADS];
  const int t = threadIdx.x;
  if (!((mask >> blockIdx.x) & 1u))
    return;
  PcgState* st = st_ + blockIdx.x;
  const double* part = part_ + (int64_t)blockIdx.x * 2 * G;
  const bool two = step == STEP_START || step == STEP_BETA || step == STEP_REPLACE;
  if (st->done && step != STEP_TRUE && step != STEP_REPLACE)
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
      st->done = 1;
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

// ---- host side -------------------------------------------------------------------------------------------------------
// the vectors of one group: R columns of n rows each, all in device memory
struct ManyWork
{
  int64_t n;
  int R;
  const double* diag;
  const uint8_t* fixed;
  double *r, *z, *d, *q, *part;
  PcgState* st;
};

inline ManyCols many_cols(const ManyWork& w, uint32_t mask, bool check)
{
  return ManyCols{w.R, mask, check ? 1 : 0, w.st};
}

inline hipError_t launch_scalar_many(const ManyWork& w, uint32_t mask, int step, double rtol, double atol,
                                     hipStream_t stream)
{
  hipLaunchKernelGGL(k_pcg_scalar_many, dim3(w.R), dim3(PS_THREADS), 0, stream, step, stream_blocks(w.n), mask,
                     static_cast<const double*>(w.part), w.st, rtol, atol);
  return hipGetLastError();
}

// JacobiSteps on columns
struct JacobiStepsMany
{
  static constexpr int check_every = PRIMAL_CHECK_EVERY;
  const ManyWork& w;
  hipStream_t stream;
  hipError_t restart(const ManyCols& c, int step, double rtol, double atol) const
  {
    hipLaunchKernelGGL(k_pcg_precond_many, dim3(stream_blocks(w.n)), dim3(PS_THREADS), 0, stream, w.n, c,
                       static_cast<const double*>(w.r), w.diag, w.fixed, w.z, w.part);
    return launch_scalar_many(w, c.mask, step, rtol, atol, stream);
  }
  hipError_t advance(const ManyCols& c, double* pu, double rtol, double atol) const
  {
    hipLaunchKernelGGL(k_pcg_update_many, dim3(stream_blocks(w.n)), dim3(PS_THREADS), 0, stream, w.n, c,
                       static_cast<const double*>(w.d), static_cast<const double*>(w.q), w.diag, w.fixed, pu, w.r, w.z,
                       w.part);
    return launch_scalar_many(w, c.mask, STEP_BETA, rtol, atol, stream);
  }
};

// pcg_solve, column by column, for one group of w.R <= MANY_R columns; b, u DEVICE [R][n], info HOST [R][8].
//   residual(cols, b, u, r, only_fixed), product(cols): the launches of pcg_solve on the columns of `cols`
//   steps: restart(cols, step, rtol, atol), advance(cols, u, rtol, atol) as JacobiStepsMany
// Every column goes the way its single solve goes.  At each read of the states the columns whose flag is set get the
// true residual; of these the ones above tolerance get the replacement and the restart, alone; a column that has
// converged, broken down or reached maxit is retired and no later launch names it.  Inside a batch a column stops at
// its own flag, so the batch may be sized by the live column with the fewest iterations left: the others go on in the
// next one.
template <class Residual, class Product, class Steps>
int pcg_solve_many(const ManyWork& w, Residual&& residual, Product&& product, const Steps& steps, const double* pb,
                   double* pu, double rtol, double atol, int32_t maxit, double* info, int32_t skipped,
                   hipStream_t stream)
{
  const int R = w.R;
  const uint32_t all = (1u << R) - 1u;
  const dim3 grid(stream_blocks(w.n)), block(PS_THREADS);
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
    note(residual(many_cols(w, mask, false), pb, pu, w.q, false));
    note(launch_scalar_many(w, mask, STEP_TRUE, rtol, atol, stream));
  };
  auto direction = [&](uint32_t mask, int first) {
    hipLaunchKernelGGL(k_pcg_direction_many, grid, block, 0, stream, w.n, many_cols(w, mask, true), first,
                       static_cast<const double*>(w.z), w.d);
    note(hipGetLastError());
  };
  note(hipMemsetAsync(w.st, 0, (size_t)R * sizeof(PcgState), stream));
  note(residual(many_cols(w, all, false), pb, pu, w.q, true));
  note(launch_scalar_many(w, all, STEP_NB, rtol, atol, stream));
  note(residual(many_cols(w, all, false), pb, pu, w.r, false));
  note(steps.restart(many_cols(w, all, false), STEP_START, rtol, atol));
  direction(all, 1);
  read_states(all);
  uint32_t live = all, nothing = 0;
  for (int c = 0; c < R; ++c)
    if (hs[c].tol == 0.0 && hs[c].nb == 0.0)
      nothing |= 1u << c;
  if (err == hipSuccess && nothing)
  {
    // nothing to solve in these columns: u^ is the solution
    hipLaunchKernelGGL(k_pcg_clear_free_many, grid, block, 0, stream, w.n, many_cols(w, nothing, false), w.fixed, pu);
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
        note(steps.restart(many_cols(w, replace, false), STEP_REPLACE, rtol, atol));
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
    const ManyCols cols = many_cols(w, live, true);
    for (int it = 0; it < batch; ++it)
    {
      note(product(cols));
      note(launch_scalar_many(w, live, STEP_ALPHA, rtol, atol, stream));
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
} // namespace
} // namespace eqlb
