// A hierarchy of refined levels ON THE DEVICE: the transpose of the P_p prolongation, the additive multilevel diagonal
// scaling (BPX) built from it, and the CG of the two primal solvers with that preconditioner - eqlb_hierarchy_* of
// include/eqlb.h.  The rule is stated there and, as numpy, in dolfinx_eqlb_amd/mesh/transfer.py: restrict_lagrange and
// dolfinx_eqlb_amd/lsolver/multilevel.py: Hierarchy; restrict and precondition reproduce the statement bit for bit.
//
// The unit owns no operator and no transfer kernel.  A level is the view its solver unit hands out (SolverLevel of
// eqlb_internal.h: diagonal, mask, slot lists behind owner_sum, residual and product launches on that unit's kernels);
// the prolongation is eqlb_refine_prolong_lagrange in device memory space (k_prolong, one launch), the store pass of the
// restriction is launch_restrict of eqlb_transfer.hip (k_restrict), its sum pass the owner sum of the COARSE handle into
// that handle's own y_loc.  What is new here are streaming kernels over the DOFs of one level:
//  k_ml_mask     r_L = r with the fixed rows set to 0
//  k_ml_combine  z = t + r / diag on the free rows, 0 on the fixed ones (t: the prolonged z of the level below; none on
//                the coarsest level); quotient and sum rounded singly, contraction off
//  k_ml_update   k_pcg_update without the fused z = r / diag: u += alpha d, r -= alpha q, block partials of r.r
//  k_ml_dot      block partials of r.z in the fixed order of the other inner products, into channel 1
//  k_ml_scalar   the scalar steps that consume r.z (start, beta, replace) with one more breakdown: r.z <= 0 or NaN;
//                the other steps are k_pcg_scalar as it is
// One application is 2 + 4 L launches on a hierarchy of L + 1 levels (mask; L store passes and L owner sums going down;
// 1 + L combines and L prolongations going up), many of them on tiny levels.  Inside a batch of iterations every kernel
// but k_prolong returns at once when the stop flag is set; the host reads the state every ML_CHECK_EVERY iterations - an
// iteration is about 4 L launches longer than a Jacobi one and the count is small, so the batch is shorter.
// All work space (r_l, z_l and the prolongation temporary t_l of every level) is carved out of one allocation at create.
// Several right-hand sides (eqlb_hierarchy_precondition_many, eqlb_hierarchy_solve_many; Poisson handles only): the
// k_ml_*_many variants below work on the columns of a ManyCols, the restriction store pass is launch_restrict_many, the
// owner sum primal_many_owner_sum, the prolongation takes the columns as its nrhs - still 2 + 4 L launches; their work
// space is grown by the first call that needs it (prepare_many).  eqlb_primal_many.h states the rule.
#include "eqlb_device_common.h"
#include "eqlb_refine_plan.h" // (eqlb_mesh_handle.h, eqlb_host_util.h)
#include "eqlb_primal_common.h" // PcgState, the scalar and vector kernels and the host loop of the CG
#include "eqlb_primal_many.h" // their column variants: several right-hand sides in one call

#include <climits>
#include <vector>

namespace eqlb
{
namespace
{
constexpr int ML_CHECK_EVERY = 8;

__global__ void __launch_bounds__(PS_THREADS)
k_ml_mask(int64_t n, const PcgState* __restrict__ st, const double* __restrict__ r, const uint8_t* __restrict__ fixed,
          double* __restrict__ out)
{
  if (st && st->done)
    return;
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x; d < n; d += (int64_t)gridDim.x * PS_THREADS)
    out[d] = fixed[d] ? 0.0 : r[d];
}

__global__ void __launch_bounds__(PS_THREADS)
k_ml_combine(int64_t n, const PcgState* __restrict__ st, const double* __restrict__ t, const double* __restrict__ r,
             const double* __restrict__ diag, const uint8_t* __restrict__ fixed, double* __restrict__ z)
{
#pragma clang fp contract(off) // the statement rounds the quotient and the sum singly
  if (st && st->done)
    return;
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x; d < n; d += (int64_t)gridDim.x * PS_THREADS)
  {
    const double jac = r[d] / diag[d];
    const double v = t ? t[d] + jac : jac;
    z[d] = fixed[d] ? 0.0 : v;
  }
}

// u += alpha d, r -= alpha q on the free rows; partials of r.r: part[0][block]
__global__ void __launch_bounds__(PS_THREADS)
k_ml_update(int64_t n, const PcgState* __restrict__ st, const double* __restrict__ p, const double* __restrict__ q,
            const uint8_t* __restrict__ fixed, double* __restrict__ u, double* __restrict__ r, double* __restrict__ part)
{
#pragma clang fp contract(off)
  __shared__ double sh[1][PS_THREADS];
  if (st->done)
    return;
  const int t = threadIdx.x;
  const double alpha = st->alpha;
  double a0 = 0.0;
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + t; d < n; d += (int64_t)gridDim.x * PS_THREADS)
  {
    if (fixed[d])
      continue; // (r is 0 there since the start)
    u[d] = u[d] + alpha * p[d];
    const double rv = r[d] - alpha * q[d];
    r[d] = rv;
    a0 = a0 + rv * rv;
  }
  sh[0][t] = a0;
  __syncthreads();
  EQLB_BLOCK_TREE_SUM(sh, t, 1, PS_THREADS)
  if (t == 0)
    part[blockIdx.x] = sh[0][0];
}

// partials of x.y: part[1][block]
__global__ void __launch_bounds__(PS_THREADS)
k_ml_dot(int64_t n, const PcgState* __restrict__ st, const double* __restrict__ x, const double* __restrict__ y,
         double* __restrict__ part)
{
#pragma clang fp contract(off)
  __shared__ double sh[1][PS_THREADS];
  if (st && st->done)
    return;
  const int t = threadIdx.x, G = gridDim.x;
  double a0 = 0.0;
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + t; d < n; d += (int64_t)G * PS_THREADS)
    a0 = a0 + x[d] * y[d];
  sh[0][t] = a0;
  __syncthreads();
  EQLB_BLOCK_TREE_SUM(sh, t, 1, PS_THREADS)
  if (t == 0)
    part[(int64_t)G + blockIdx.x] = sh[0][0];
}

// STEP_START, STEP_BETA, STEP_REPLACE of k_pcg_scalar for a preconditioner that is not a positive diagonal: the same
// totals by the same tree, the same moves of the state, and breakdown where the iteration would go on with r.z <= 0
__global__ void __launch_bounds__(PS_THREADS)
k_ml_scalar(int step, int G, const double* __restrict__ part, PcgState* __restrict__ st)
{
  __shared__ double sh[2][PS_THREADS];
  const int t = threadIdx.x;
  if (st->done && step != STEP_REPLACE)
    return;
#pragma unroll
  for (int j = 0; j < 2; ++j)
  {
    double a = 0.0;
    for (int b = t; b < G; b += PS_THREADS)
      a += part[(int64_t)j * G + b];
    sh[j][t] = a;
  }
  __syncthreads();
  EQLB_BLOCK_TREE_SUM(sh, t, 2, PS_THREADS)
  if (t != 0)
    return;
  const double s0 = sh[0][0], s1 = sh[1][0];
  st->rr = s0;
  bool goes_on = true;
  if (step == STEP_START)
  {
    st->rho = s1;
    goes_on = !(sqrt(s0) <= st->tol);
    st->done = goes_on ? 0 : 1;
  }
  else if (step == STEP_BETA)
  {
    st->iters += 1;
    goes_on = !(sqrt(s0) <= st->tol);
    if (goes_on)
    {
      st->beta = s1 / st->rho;
      st->rho = s1;
    }
    else
      st->done = 1; // (rho stays that of the last direction: STEP_REPLACE needs it if the true residual is above tol)
  }
  else // STEP_REPLACE
  {
    st->beta = s1 / st->rho;
    st->rho = s1;
    st->replacements += 1;
    st->done = 0;
  }
  if (goes_on && !(s1 > 0.0))
  {
    st->breakdown = 1;
    st->done = 1;
  }
}

// ---- the same kernels on columns (eqlb_hierarchy_*_many; eqlb_primal_many.h states the rule): one thread per DOF
// carries the values of that DOF in the columns of its ManyCols, vectors [R][n], partials [R][2][G] ------------------
__global__ void __launch_bounds__(PS_THREADS)
k_ml_mask_many(int64_t n, const ManyCols cols, const double* __restrict__ r, const uint8_t* __restrict__ fixed,
               double* __restrict__ out)
{
  const uint32_t live = many_live(cols);
  if (!live)
    return;
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x; d < n; d += (int64_t)gridDim.x * PS_THREADS)
  {
    const bool fx = fixed[d];
#pragma unroll
    for (int k = 0; k < MANY_R; ++k)
      if ((live >> k) & 1u)
        out[k * n + d] = fx ? 0.0 : r[k * n + d];
  }
}

__global__ void __launch_bounds__(PS_THREADS)
k_ml_combine_many(int64_t n, const ManyCols cols, const double* __restrict__ t, const double* __restrict__ r,
                  const double* __restrict__ diag, const uint8_t* __restrict__ fixed, double* __restrict__ z)
{
#pragma clang fp contract(off) // the statement rounds the quotient and the sum singly
  const uint32_t live = many_live(cols);
  if (!live)
    return;
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x; d < n; d += (int64_t)gridDim.x * PS_THREADS)
  {
    const bool fx = fixed[d];
    const double dg = diag[d];
#pragma unroll
    for (int k = 0; k < MANY_R; ++k)
    {
      if (!((live >> k) & 1u))
        continue;
      const double jac = r[k * n + d] / dg;
      const double v = t ? t[k * n + d] + jac : jac;
      z[k * n + d] = fx ? 0.0 : v;
    }
  }
}

// partials of r.r of column k: part[2 k][block]
__global__ void __launch_bounds__(PS_THREADS)
k_ml_update_many(int64_t n, const ManyCols cols, const double* __restrict__ p, const double* __restrict__ q,
                 const uint8_t* __restrict__ fixed, double* __restrict__ u, double* __restrict__ r,
                 double* __restrict__ part)
{
#pragma clang fp contract(off)
  __shared__ double sh[MANY_R][PS_THREADS];
  const uint32_t live = many_live(cols);
  if (!live)
    return;
  const PcgState* st = static_cast<const PcgState*>(cols.st);
  const int t = threadIdx.x;
  double alpha[MANY_R];
#pragma unroll
  for (int k = 0; k < MANY_R; ++k)
    alpha[k] = ((live >> k) & 1u) ? st[k].alpha : 0.0;
  double a0[MANY_R] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + t; d < n; d += (int64_t)gridDim.x * PS_THREADS)
  {
    if (fixed[d])
      continue; // (r is 0 there since the start)
#pragma unroll
    for (int k = 0; k < MANY_R; ++k)
    {
      if (!((live >> k) & 1u))
        continue;
      const int64_t e = k * n + d;
      u[e] = u[e] + alpha[k] * p[e];
      const double rv = r[e] - alpha[k] * q[e];
      r[e] = rv;
      a0[k] = a0[k] + rv * rv;
    }
  }
#pragma unroll
  for (int k = 0; k < MANY_R; ++k)
    sh[k][t] = a0[k];
  __syncthreads();
  EQLB_BLOCK_TREE_SUM(sh, t, MANY_R, PS_THREADS)
  if (t < MANY_R && ((live >> t) & 1u))
    part[(int64_t)(2 * t) * gridDim.x + blockIdx.x] = sh[t][0];
}

// partials of x.y of column k: part[2 k + 1][block]
__global__ void __launch_bounds__(PS_THREADS)
k_ml_dot_many(int64_t n, const ManyCols cols, const double* __restrict__ x, const double* __restrict__ y,
              double* __restrict__ part)
{
#pragma clang fp contract(off)
  __shared__ double sh[MANY_R][PS_THREADS];
  const uint32_t live = many_live(cols);
  if (!live)
    return;
  const int t = threadIdx.x, G = gridDim.x;
  double a0[MANY_R] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + t; d < n; d += (int64_t)G * PS_THREADS)
  {
#pragma unroll
    for (int k = 0; k < MANY_R; ++k)
      if ((live >> k) & 1u)
        a0[k] = a0[k] + x[k * n + d] * y[k * n + d];
  }
#pragma unroll
  for (int k = 0; k < MANY_R; ++k)
    sh[k][t] = a0[k];
  __syncthreads();
  EQLB_BLOCK_TREE_SUM(sh, t, MANY_R, PS_THREADS)
  if (t < MANY_R && ((live >> t) & 1u))
    part[(int64_t)(2 * t + 1) * G + blockIdx.x] = sh[t][0];
}

// k_ml_scalar, one block per column of mask
__global__ void __launch_bounds__(PS_THREADS)
k_ml_scalar_many(int step, int G, uint32_t mask, const double* __restrict__ part_, PcgState* __restrict__ st_)
{
  __shared__ double sh[2][PS_THREADS];
  const int t = threadIdx.x;
  if (!((mask >> blockIdx.x) & 1u))
    return;
  PcgState* st = st_ + blockIdx.x;
  const double* part = part_ + (int64_t)blockIdx.x * 2 * G;
  if (st->done && step != STEP_REPLACE)
    return;
#pragma unroll
  for (int j = 0; j < 2; ++j)
  {
    double a = 0.0;
    for (int b = t; b < G; b += PS_THREADS)
      a += part[(int64_t)j * G + b];
    sh[j][t] = a;
  }
  __syncthreads();
  EQLB_BLOCK_TREE_SUM(sh, t, 2, PS_THREADS)
  if (t != 0)
    return;
  const double s0 = sh[0][0], s1 = sh[1][0];
  st->rr = s0;
  bool goes_on = true;
  if (step == STEP_START)
  {
    st->rho = s1;
    goes_on = !(sqrt(s0) <= st->tol);
    st->done = goes_on ? 0 : 1;
  }
  else if (step == STEP_BETA)
  {
    st->iters += 1;
    goes_on = !(sqrt(s0) <= st->tol);
    if (goes_on)
    {
      st->beta = s1 / st->rho;
      st->rho = s1;
    }
    else
      st->done = 1;
  }
  else // STEP_REPLACE
  {
    st->beta = s1 / st->rho;
    st->rho = s1;
    st->replacements += 1;
    st->done = 0;
  }
  if (goes_on && !(s1 > 0.0))
  {
    st->breakdown = 1;
    st->done = 1;
  }
}
} // namespace
} // namespace eqlb

// the handle behind eqlb_hierarchy_t: views of the borrowed levels and the work space
struct eqlb_hierarchy
{
  int nlevels = 0, bs = 0, p = 0;
  std::vector<eqlb::SolverLevel> lv;
  std::vector<eqlb_refine*> plans;
  std::vector<int64_t> n; // bs * ndofs per level
  eqlb::DevCarve mem;
  std::vector<eqlb::DevPiece<double>> r, z, t;
  // the *_many entries: r_l, z_l, t_l for many_R columns, grown by the first call that needs them; the views of the
  // levels' own work space for columns, read anew by every call
  int many_R = 0;
  eqlb::DevBuf<char> many_mem;
  std::vector<double*> mr, mz, mt;
  std::vector<eqlb::ManyLevel> mlv;
};

namespace eqlb
{
namespace
{
// level + 1 -> level: the store pass into the y_loc of the coarse handle, then its owner sum
int enqueue_restrict(const char* who, const eqlb_hierarchy& h, int level, const double* r_fine, double* r_coarse,
                     bool masked, const PcgState* st, hipStream_t stream)
{
  const SolverLevel &lo = h.lv[level], &hi = h.lv[level + 1];
  EQLB_TRY(launch_restrict(who, h.plans[level], hi.mesh, h.p, h.bs, hi.cell_dofs, hi.ndofs, r_fine, lo.yloc,
                           st ? &st->done : nullptr, stream));
  HIP_TRY(lo.owner_sum(lo.handle, r_coarse, masked, st, stream));
  return EQLB_OK;
}

// z = M r on the finest level; r, z DEVICE
int enqueue_precondition(const char* who, const eqlb_hierarchy& h, const double* r, double* z, const PcgState* st,
                         hipStream_t stream)
{
  const int L = h.nlevels - 1;
  const dim3 block(PS_THREADS);
  if (L == 0)
  {
    hipLaunchKernelGGL(k_ml_combine, dim3(stream_blocks(h.n[0])), block, 0, stream, h.n[0], st,
                       static_cast<const double*>(nullptr), r, h.lv[0].diag, h.lv[0].fixed, z);
    HIP_TRY(hipGetLastError());
    return EQLB_OK;
  }
  hipLaunchKernelGGL(k_ml_mask, dim3(stream_blocks(h.n[L])), block, 0, stream, h.n[L], st, r, h.lv[L].fixed,
                     h.r[L].get());
  HIP_TRY(hipGetLastError());
  for (int l = L - 1; l >= 0; --l)
    EQLB_TRY(enqueue_restrict(who, h, l, h.r[l + 1], h.r[l], true, st, stream));
  hipLaunchKernelGGL(k_ml_combine, dim3(stream_blocks(h.n[0])), block, 0, stream, h.n[0], st,
                     static_cast<const double*>(nullptr), static_cast<const double*>(h.r[0].get()), h.lv[0].diag,
                     h.lv[0].fixed, h.z[0].get());
  HIP_TRY(hipGetLastError());
  for (int l = 1; l <= L; ++l)
  {
    // (k_prolong knows no stop flag: inside a finished batch it prolongs a z_l nobody reads)
    EQLB_TRY(eqlb_refine_prolong_lagrange(h.plans[l - 1], h.lv[l].mesh, h.p, h.bs, 1, h.lv[l - 1].cell_dofs,
                                          h.lv[l - 1].ndofs, h.z[l - 1], h.lv[l].cell_dofs, h.lv[l].ndofs, h.t[l],
                                          EQLB_MEM_DEVICE, stream));
    hipLaunchKernelGGL(k_ml_combine, dim3(stream_blocks(h.n[l])), block, 0, stream, h.n[l], st,
                       static_cast<const double*>(h.t[l].get()), static_cast<const double*>(h.r[l].get()), h.lv[l].diag,
                       h.lv[l].fixed, l == L ? z : h.z[l].get());
    HIP_TRY(hipGetLastError());
  }
  return EQLB_OK;
}

// the preconditioner inside pcg_solve (eqlb_primal_common.h: JacobiSteps is the counterpart)
struct MultilevelSteps
{
  static constexpr int check_every = ML_CHECK_EVERY;
  const eqlb_hierarchy& h;
  const PcgWork& w;
  hipStream_t stream;
  hipError_t rz_and_scalar(int step, const PcgState* st) const
  {
    const int G = stream_blocks(w.n);
    hipLaunchKernelGGL(k_ml_dot, dim3(G), dim3(PS_THREADS), 0, stream, w.n, st, static_cast<const double*>(w.r),
                       static_cast<const double*>(w.z), w.part);
    hipLaunchKernelGGL(k_ml_scalar, dim3(1), dim3(PS_THREADS), 0, stream, step, G, static_cast<const double*>(w.part),
                       w.st);
    return hipGetLastError();
  }
  // (the residual launch has left the partials of r.r in channel 0)
  hipError_t restart(int step, double, double) const
  {
    if (enqueue_precondition("eqlb_hierarchy_solve", h, w.r, w.z, nullptr, stream) != EQLB_OK)
      return hipErrorUnknown;
    return rz_and_scalar(step, nullptr);
  }
  hipError_t advance(double* pu, double, double) const
  {
    hipLaunchKernelGGL(k_ml_update, dim3(stream_blocks(w.n)), dim3(PS_THREADS), 0, stream, w.n,
                       static_cast<const PcgState*>(w.st), static_cast<const double*>(w.d),
                       static_cast<const double*>(w.q), w.fixed, pu, w.r, w.part);
    if (enqueue_precondition("eqlb_hierarchy_solve", h, w.r, w.z, w.st, stream) != EQLB_OK)
      return hipErrorUnknown;
    return rz_and_scalar(STEP_BETA, w.st);
  }
};

// ---- several right-hand sides ----------------------------------------------------------------------------------------
// what every *_many entry checks, and the work space for R columns: r_l, z_l, t_l here, y_loc (and, on the finest
// level, the vectors of the CG) in the solver handles
int prepare_many(const char* who, eqlb_hierarchy* h, int32_t nrhs, const void* a, const void* b, int32_t memspace)
{
  if (!h || !a || !b)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  if (nrhs < 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: nrhs = %d (at least 1)", who, (int)nrhs);
  if (h->bs != 1)
    return fail(EQLB_ERR_UNSUPPORTED, "%s: several right-hand sides are provided for Poisson handles (bs = 1) only", who);
  EQLB_TRY(check_memspace(who, memspace));
  const int R = nrhs < MANY_R ? nrhs : MANY_R;
  h->mlv.resize(h->nlevels);
  for (int l = 0; l < h->nlevels; ++l)
    EQLB_TRY(primal_many_level(static_cast<eqlb_primal*>(h->lv[l].handle), R, h->mlv[l]));
  if (R > h->many_R && h->nlevels > 1)
  {
    std::vector<size_t> off(3 * h->nlevels);
    size_t bytes = 0;
    for (int l = 0; l < h->nlevels; ++l)
      for (int j = 0; j < 3; ++j)
      {
        off[3 * l + j] = bytes;
        bytes += round_up256((size_t)R * h->n[l] * sizeof(double));
      }
    h->many_R = 0;
    HIP_TRY(h->many_mem.alloc_raw(bytes)); // (frees the smaller one first)
    h->mr.resize(h->nlevels);
    h->mz.resize(h->nlevels);
    h->mt.resize(h->nlevels);
    for (int l = 0; l < h->nlevels; ++l)
    {
      h->mr[l] = reinterpret_cast<double*>(h->many_mem.get() + off[3 * l]);
      h->mz[l] = reinterpret_cast<double*>(h->many_mem.get() + off[3 * l + 1]);
      h->mt[l] = reinterpret_cast<double*>(h->many_mem.get() + off[3 * l + 2]);
    }
    h->many_R = R;
  }
  return EQLB_OK;
}

// enqueue_precondition on the columns of c: r, z DEVICE [R][n_L]; 2 + 4 L launches whatever R is
int enqueue_precondition_many(const char* who, const eqlb_hierarchy& h, const ManyCols& c, const double* r, double* z,
                              hipStream_t stream)
{
  const int L = h.nlevels - 1;
  const dim3 block(PS_THREADS);
  const double* const none = nullptr;
  if (L == 0)
  {
    hipLaunchKernelGGL(k_ml_combine_many, dim3(stream_blocks(h.n[0])), block, 0, stream, h.n[0], c, none, r,
                       h.lv[0].diag, h.lv[0].fixed, z);
    HIP_TRY(hipGetLastError());
    return EQLB_OK;
  }
  const PcgState* st = static_cast<const PcgState*>(c.st);
  const int32_t* done0 = (c.check && st) ? &st->done : nullptr;
  constexpr int done_stride = (int)(sizeof(PcgState) / sizeof(int32_t));
  hipLaunchKernelGGL(k_ml_mask_many, dim3(stream_blocks(h.n[L])), block, 0, stream, h.n[L], c, r, h.lv[L].fixed,
                     h.mr[L]);
  HIP_TRY(hipGetLastError());
  for (int l = L - 1; l >= 0; --l)
  {
    const SolverLevel &lo = h.lv[l], &hi = h.lv[l + 1];
    EQLB_TRY(launch_restrict_many(who, h.plans[l], hi.mesh, h.p, c.R, c.mask, hi.cell_dofs, hi.ndofs, h.mr[l + 1],
                                  h.mlv[l].yloc, done0, done_stride, stream));
    HIP_TRY(primal_many_owner_sum(static_cast<eqlb_primal*>(lo.handle), c, h.mr[l], true, stream));
  }
  hipLaunchKernelGGL(k_ml_combine_many, dim3(stream_blocks(h.n[0])), block, 0, stream, h.n[0], c, none,
                     static_cast<const double*>(h.mr[0]), h.lv[0].diag, h.lv[0].fixed, h.mz[0]);
  HIP_TRY(hipGetLastError());
  for (int l = 1; l <= L; ++l)
  {
    // (k_prolong knows no columns to leave out: it prolongs all R, into a t_l whose idle columns nobody reads)
    EQLB_TRY(eqlb_refine_prolong_lagrange(h.plans[l - 1], h.lv[l].mesh, h.p, 1, c.R, h.lv[l - 1].cell_dofs,
                                          h.lv[l - 1].ndofs, h.mz[l - 1], h.lv[l].cell_dofs, h.lv[l].ndofs, h.mt[l],
                                          EQLB_MEM_DEVICE, stream));
    hipLaunchKernelGGL(k_ml_combine_many, dim3(stream_blocks(h.n[l])), block, 0, stream, h.n[l], c,
                       static_cast<const double*>(h.mt[l]), static_cast<const double*>(h.mr[l]), h.lv[l].diag,
                       h.lv[l].fixed, l == L ? z : h.mz[l]);
    HIP_TRY(hipGetLastError());
  }
  return EQLB_OK;
}

// MultilevelSteps on columns
struct MultilevelStepsMany
{
  static constexpr int check_every = ML_CHECK_EVERY;
  const eqlb_hierarchy& h;
  const ManyWork& w;
  hipStream_t stream;
  hipError_t rz_and_scalar(const ManyCols& c, int step) const
  {
    const int G = stream_blocks(w.n);
    hipLaunchKernelGGL(k_ml_dot_many, dim3(G), dim3(PS_THREADS), 0, stream, w.n, c, static_cast<const double*>(w.r),
                       static_cast<const double*>(w.z), w.part);
    hipLaunchKernelGGL(k_ml_scalar_many, dim3(w.R), dim3(PS_THREADS), 0, stream, step, G, c.mask,
                       static_cast<const double*>(w.part), w.st);
    return hipGetLastError();
  }
  hipError_t restart(const ManyCols& c, int step, double, double) const
  {
    if (enqueue_precondition_many("eqlb_hierarchy_solve_many", h, c, w.r, w.z, stream) != EQLB_OK)
      return hipErrorUnknown;
    return rz_and_scalar(c, step);
  }
  hipError_t advance(const ManyCols& c, double* pu, double, double) const
  {
    hipLaunchKernelGGL(k_ml_update_many, dim3(stream_blocks(w.n)), dim3(PS_THREADS), 0, stream, w.n, c,
                       static_cast<const double*>(w.d), static_cast<const double*>(w.q), w.fixed, pu, w.r, w.part);
    if (enqueue_precondition_many("eqlb_hierarchy_solve_many", h, c, w.r, w.z, stream) != EQLB_OK)
      return hipErrorUnknown;
    return rz_and_scalar(c, STEP_BETA);
  }
};
} // namespace
} // namespace eqlb

extern "C" {

int eqlb_hierarchy_create(int32_t nlevels, int32_t bs, void* const* solvers, eqlb_refine_t* const* plans,
                          eqlb_mesh_t* const* meshes, void* stream_, eqlb_hierarchy_t** out)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_hierarchy_create";
  (void)stream_; // (nothing is enqueued: the work space is written before it is read)
  if (nlevels < 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: nlevels = %d (at least 1)", who, (int)nlevels);
  if (bs != 1 && bs != 2)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: bs = %d is not 1 (eqlb_primal_t) or 2 (eqlb_elasticity_t)", who, (int)bs);
  if (!solvers || !meshes || !out || (nlevels > 1 && !plans))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  for (int l = 0; l < nlevels; ++l)
    if (!solvers[l] || !meshes[l] || (l < nlevels - 1 && !plans[l]))
      return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument (level %d)", who, l);
  std::unique_ptr<eqlb_hierarchy> h(new eqlb_hierarchy);
  h->nlevels = nlevels;
  h->bs = bs;
  h->lv.resize(nlevels);
  for (int l = 0; l < nlevels; ++l)
  {
    if (bs == 1)
      primal_level(static_cast<eqlb_primal*>(solvers[l]), h->lv[l]);
    else
      elasticity_level(static_cast<eqlb_elasticity*>(solvers[l]), h->lv[l]);
    const SolverLevel& v = h->lv[l];
    if (v.p != h->lv[0].p)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: levels of different p: %d on level 0, %d on level %d", who,
                  h->lv[0].p, v.p, l);
    const DeviceMesh &sm = v.mesh->m, &lm = meshes[l]->m;
    if (sm.nnodes != lm.nnodes || sm.ncells != lm.ncells || sm.nfacets != lm.nfacets)
      return fail(EQLB_ERR_INVALID_ARGUMENT,
                  "%s: the solver of level %d stands on a mesh of %d nodes and %d cells, the level has %d and %d", who, l,
                  sm.nnodes, sm.ncells, lm.nnodes, lm.ncells);
  }
  h->p = h->lv[0].p;
  for (int l = 0; l + 1 < nlevels; ++l)
  {
    const eqlb_refine& pl = *plans[l];
    const DeviceMesh &m0 = meshes[l]->m, &m1 = meshes[l + 1]->m;
    if (pl.nnodes != m0.nnodes || pl.ncells != m0.ncells || pl.nfacets != m0.nfacets)
      return fail(EQLB_ERR_INVALID_ARGUMENT,
                  "%s: plan %d refines a mesh of %d nodes and %d cells, level %d has %d and %d", who, l, pl.nnodes,
                  pl.ncells, l, m0.nnodes, m0.ncells);
    if (pl.nnodes + pl.nbis != m1.nnodes || pl.ncells2 != m1.ncells)
      return fail(EQLB_ERR_INVALID_ARGUMENT,
                  "%s: plan %d gives a mesh of %d nodes and %d cells, level %d has %d and %d", who, l,
                  pl.nnodes + pl.nbis, pl.ncells2, l + 1, m1.nnodes, m1.ncells);
    h->plans.push_back(plans[l]);
  }
  h->n.resize(nlevels);
  h->r.resize(nlevels);
  h->z.resize(nlevels);
  h->t.resize(nlevels);
  for (int l = 0; l < nlevels; ++l)
  {
    h->n[l] = h->lv[l].ndofs * bs;
    if (nlevels == 1)
      break; // (plain Jacobi works on the caller's vectors)
    h->r[l] = h->mem.piece<double>((size_t)h->n[l]);
    if (l < nlevels - 1)
      h->z[l] = h->mem.piece<double>((size_t)h->n[l]);
    if (l > 0)
      h->t[l] = h->mem.piece<double>((size_t)h->n[l]);
  }
  HIP_TRY(h->mem.alloc());
  *out = h.release();
  return EQLB_OK;
}
EQLB_CATCH_ALL

void eqlb_hierarchy_destroy(eqlb_hierarchy_t* handle) { delete handle; }

int eqlb_hierarchy_restrict(eqlb_hierarchy_t* h, int32_t level, const double* r_fine, double* r_coarse, int32_t masked,
                            int32_t memspace, void* stream_)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_hierarchy_restrict";
  if (!h || !r_fine || !r_coarse)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  if (level < 0 || level > h->nlevels - 2)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: level = %d outside 0 ... %d (the restriction goes from level + 1 to level)",
                who, (int)level, h->nlevels - 2);
  EQLB_TRY(check_memspace(who, memspace));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool host = memspace == EQLB_MEM_HOST;
  HostCall s;
  const auto d_in = s.in(host ? r_fine : nullptr, (size_t)h->n[level + 1]);
  const auto d_out = s.out(host ? r_coarse : nullptr, (size_t)h->n[level]);
  if (host)
    HIP_TRY(s.upload(stream));
  const int st = enqueue_restrict(who, *h, level, host ? d_in.get() : r_fine, host ? d_out.get() : r_coarse,
                                  masked != 0, nullptr, stream);
  HIP_TRY(s.finish(stream));
  return st;
}
EQLB_CATCH_ALL

int eqlb_hierarchy_precondition(eqlb_hierarchy_t* h, const double* r, double* z, int32_t memspace, void* stream_)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_hierarchy_precondition";
  if (!h || !r || !z)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  EQLB_TRY(check_memspace(who, memspace));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool host = memspace == EQLB_MEM_HOST;
  const size_t n = (size_t)h->n[h->nlevels - 1];
  HostCall s;
  const auto d_r = s.in(host ? r : nullptr, n);
  const auto d_z = s.out(host ? z : nullptr, n);
  if (host)
    HIP_TRY(s.upload(stream));
  const int st = enqueue_precondition(who, *h, host ? d_r.get() : r, host ? d_z.get() : z, nullptr, stream);
  HIP_TRY(s.finish(stream));
  return st;
}
EQLB_CATCH_ALL

int eqlb_hierarchy_solve(eqlb_hierarchy_t* h, const double* b, double* u, double rtol, double atol, int32_t maxit,
                         double* info, int32_t memspace, void* stream_)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_hierarchy_solve";
  if (maxit < 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: maxit = %d (at least 1)", who, (int)maxit);
  if (!(rtol >= 0.0) || !(atol >= 0.0))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: rtol = %g, atol = %g negative or NaN", who, rtol, atol);
  if (!h || !b || !u || !info)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  EQLB_TRY(check_memspace(who, memspace));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const SolverLevel& top = h->lv[h->nlevels - 1];
  // the status word of the finest mask: the call waits by nature, and nothing is launched for a singular problem
  int32_t status[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(status, top.status, sizeof(status), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  for (int c = 0; c < h->bs; ++c)
    if (status[1 + c] < 1)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: singular: component %d of the finest level has no Dirichlet DOF", who,
                  c);
  const PcgWork w{h->n[h->nlevels - 1], top.diag, top.fixed, top.r, top.z,
                  top.d,                top.q,    top.part,  static_cast<PcgState*>(top.st)};
  auto residual = [&](const double* pb, const double* pu, double* r, bool only_fixed) {
    return top.residual(top.handle, pb, pu, r, only_fixed, stream);
  };
  auto product = [&](const PcgState*) { return top.product(top.handle, stream); };
  return pcg_solve(w, residual, product, MultilevelSteps{*h, w, stream}, b, u, rtol, atol, maxit, info, status[0],
                   memspace == EQLB_MEM_HOST, stream);
}
EQLB_CATCH_ALL

int eqlb_hierarchy_precondition_many(eqlb_hierarchy_t* h, int32_t nrhs, const double* r, double* z, int32_t memspace,
                                     void* stream_)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_hierarchy_precondition_many";
  EQLB_TRY(prepare_many(who, h, nrhs, r, z, memspace));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool host = memspace == EQLB_MEM_HOST;
  const size_t n = (size_t)h->n[h->nlevels - 1];
  HostCall s;
  const auto d_r = s.in(host ? r : nullptr, nrhs * n);
  const auto d_z = s.out(host ? z : nullptr, nrhs * n);
  if (host)
    HIP_TRY(s.upload(stream));
  const double* pr = host ? d_r.get() : r;
  double* pz = host ? d_z.get() : z;
  int st = EQLB_OK;
  for (int32_t c0 = 0; c0 < nrhs && st == EQLB_OK; c0 += MANY_R)
  {
    const int R = nrhs - c0 < MANY_R ? nrhs - c0 : MANY_R;
    st = enqueue_precondition_many(who, *h, ManyCols{R, (1u << R) - 1u, 0, nullptr}, pr + c0 * n, pz + c0 * n, stream);
  }
  HIP_TRY(s.finish(stream));
  return st;
}
EQLB_CATCH_ALL

int eqlb_hierarchy_solve_many(eqlb_hierarchy_t* h, int32_t nrhs, const double* b, double* u, double rtol, double atol,
                              int32_t maxit, double* info, int32_t memspace, void* stream_)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_hierarchy_solve_many";
  if (maxit < 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: maxit = %d (at least 1)", who, (int)maxit);
  if (!(rtol >= 0.0) || !(atol >= 0.0))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: rtol = %g, atol = %g negative or NaN", who, rtol, atol);
  if (!info)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  EQLB_TRY(prepare_many(who, h, nrhs, b, u, memspace));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const SolverLevel& top = h->lv[h->nlevels - 1];
  eqlb_primal* const th = static_cast<eqlb_primal*>(top.handle);
  // the status word of the finest mask: the call waits by nature, and nothing is launched for a singular problem
  int32_t status[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(status, top.status, sizeof(status), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  if (status[1] < 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: singular: the finest level has no Dirichlet DOF", who);
  const bool host = memspace == EQLB_MEM_HOST;
  const size_t n = (size_t)h->n[h->nlevels - 1];
  HostCall s;
  const auto d_b = s.in(host ? b : nullptr, nrhs * n);
  const auto d_u = s.in(host ? static_cast<const double*>(u) : nullptr, nrhs * n);
  if (host)
    HIP_TRY(s.upload(stream));
  const double* pb = host ? d_b.get() : b;
  double* pu = host ? d_u.get() : u;
  auto residual = [&](const ManyCols& c, const double* xb, const double* xu, double* r, bool only_fixed) {
    return primal_many_residual(th, c, xb, xu, r, only_fixed, stream);
  };
  auto product = [&](const ManyCols& c) { return primal_many_product(th, c, stream); };
  const ManyLevel& tv = h->mlv[h->nlevels - 1];
  for (int32_t c0 = 0; c0 < nrhs; c0 += MANY_R)
  {
    const ManyWork w{(int64_t)n, nrhs - c0 < MANY_R ? (int)(nrhs - c0) : MANY_R, top.diag, top.fixed, tv.r, tv.z, tv.d,
                     tv.q,       tv.part, static_cast<PcgState*>(tv.st)};
    EQLB_TRY(pcg_solve_many(w, residual, product, MultilevelStepsMany{*h, w, stream}, pb + c0 * n, pu + c0 * n, rtol,
                            atol, maxit, info + 8 * (size_t)c0, status[0], stream));
  }
  if (host)
    s.out_prefix(u, d_u, nrhs * n);
  HIP_TRY(s.finish(stream));
  return EQLB_OK;
}
EQLB_CATCH_ALL

} // extern "C"
