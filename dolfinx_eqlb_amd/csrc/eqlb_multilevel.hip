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
//  k_ml_combine_local  the same with the mask of the local rule: a free row that is not active on its level takes t as it
//                is - no quotient, no addition; r and diag are read on the active rows only
//  k_ml_update   k_pcg_update without the fused z = r / diag: u += alpha d, r -= alpha q, block partials of r.r
//  k_ml_dot      block partials of r.z in the fixed order of the other inner products, into channel 1
// The scalar steps are k_pcg_scalar; those that consume r.z (start, beta, replace) run with its `ml` flag: one more
// breakdown, r.z <= 0 or NaN.
// One application is 2 + 4 L launches on a hierarchy of L + 1 levels (mask; L store passes and L owner sums going down;
// 1 + L combines and L prolongations going up), many of them on tiny levels.  Inside a batch of iterations every kernel
// but k_prolong leaves a column alone when its stop flag is set; the host reads the states every ML_CHECK_EVERY
// iterations - an iteration is about 4 L launches longer than a Jacobi one and the count is small, so the batch is
// shorter.
// Several right-hand sides (eqlb_hierarchy_precondition_many, eqlb_hierarchy_solve_many; Poisson handles only) run on
// the same kernels and the same host code, as eqlb_primal_common.h states it: every kernel here has NC column slots and
// works on the columns of a ManyCols, the prolongation takes the columns as its nrhs - still 2 + 4 L launches.  The work
// space for one column (r_l, z_l and the prolongation temporary t_l of every level) is carved out of one allocation at
// create; the one for more columns is grown by the first call that needs it (prepare).
// Local smoothing (eqlb_hierarchy_set_local; the rule: the head of lsolver/multilevel.py): a mask uint8 [bs ndofs_l] per
// level l >= 1, owned by the handle, written by k_ml_active from the parent-to-children table the plan of link l - 1
// keeps for k_prolong and k_restrict (coff) and the dofmap of level l.  With the switch on, the combines of the levels
// l >= 1 are k_ml_combine_local; the launches of an application stay 2 + 4 L, and with the switch off they are the
// launches of a handle that never saw the switch.
// Exact solve on level 0 (eqlb_hierarchy_set_coarse; the rule: the head of lsolver/multilevel.py; the factor and the two
// kernels of its application: eqlb_coarse.hip).  With the switch on, the combine of level 0 is not launched: the two
// launches of coarse_apply stand in its place, and an application is 3 + 4 L launches.  With the switch off the
// launches are those of a handle that never saw the switch.
#include "eqlb_device_common.h"
#include "eqlb_coarse.h"
#include "eqlb_refine_plan.h" // (eqlb_mesh_handle.h, eqlb_host_util.h)
#include "eqlb_primal_common.h" // PcgState, the scalar and vector kernels and the host loop of the CG

#include <algorithm>
#include <climits>
#include <vector>

namespace eqlb
{
namespace
{
constexpr int ML_CHECK_EVERY = 8;

// one thread per DOF carries the values of that DOF in the columns of its ManyCols: vectors [R][n], partials [R][2][G]
template <int NC>
__global__ void __launch_bounds__(PS_THREADS)
k_ml_mask(int64_t n, const ManyCols cols, const double* __restrict__ r, const uint8_t* __restrict__ fixed,
          double* __restrict__ out)
{
  const uint32_t live = cols_live<NC>(cols);
  if (!live)
    return;
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x; d < n; d += (int64_t)gridDim.x * PS_THREADS)
  {
    const bool fx = fixed[d];
#pragma unroll
    for (int k = 0; k < NC; ++k)
      if (col_on<NC>(live, k))
        out[k * n + d] = fx ? 0.0 : r[k * n + d];
  }
}

template <int NC>
__global__ void __launch_bounds__(PS_THREADS)
k_ml_combine(int64_t n, const ManyCols cols, const double* __restrict__ t, const double* __restrict__ r,
             const double* __restrict__ diag, const uint8_t* __restrict__ fixed, double* __restrict__ z)
{
#pragma clang fp contract(off) // the statement rounds the quotient and the sum singly
  const uint32_t live = cols_live<NC>(cols);
  if (!live)
    return;
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x; d < n; d += (int64_t)gridDim.x * PS_THREADS)
  {
    const bool fx = fixed[d];
    const double dg = diag[d];
#pragma unroll
    for (int k = 0; k < NC; ++k)
    {
      if (!col_on<NC>(live, k))
        continue;
      const double jac = r[k * n + d] / dg;
      const double v = t ? t[k * n + d] + jac : jac;
      z[k * n + d] = fx ? 0.0 : v;
    }
  }
}

// the combine of a level l >= 1 under the local rule: t is there, and so is the mask of the level
template <int NC>
__global__ void __launch_bounds__(PS_THREADS)
k_ml_combine_local(int64_t n, const ManyCols cols, const double* __restrict__ t, const double* __restrict__ r,
                   const double* __restrict__ diag, const uint8_t* __restrict__ fixed,
                   const uint8_t* __restrict__ active, double* __restrict__ z)
{
#pragma clang fp contract(off) // the statement rounds the quotient and the sum singly
  const uint32_t live = cols_live<NC>(cols);
  if (!live)
    return;
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x; d < n; d += (int64_t)gridDim.x * PS_THREADS)
  {
    const bool fx = fixed[d];
    const bool on = !fx && active[d];
    const double dg = on ? diag[d] : 1.0;
#pragma unroll
    for (int k = 0; k < NC; ++k)
    {
      if (!col_on<NC>(live, k))
        continue;
      double v = 0.0;
      if (!fx)
      {
        v = t[k * n + d];
        if (on)
          v = v + r[k * n + d] / dg;
      }
      z[k * n + d] = v;
    }
  }
}

// The mask of one level l >= 1: one thread per cell of the level below, which walks its children - the fine cells, in
// the order k_restrict walks them.  The children of a bisected cell (more than one child) write 1 to the bs rows of
// every DOF of their row of the dofmap: the same byte from several threads, plain stores, no atomics (k_primal_mask
// does the same).  The mask is cleared before the launch; an index outside the level addresses nothing.
__global__ void __launch_bounds__(PS_THREADS)
k_ml_active(int32_t ncells, int64_t ncells2, const uint32_t* __restrict__ coff, int nd, int bs,
            const int32_t* __restrict__ cell_dofs2, int64_t ndofs2, uint8_t* __restrict__ active)
{
  const int64_t c = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (c >= ncells)
    return;
  const int64_t first = coff[c], last = coff[c + 1];
  if (last - first < 2 || last > ncells2)
    return;
  for (int64_t c2 = first; c2 < last; ++c2)
    for (int i = 0; i < nd; ++i)
    {
      const int64_t d = cell_dofs2[c2 * nd + i];
      if (d < 0 || d >= ndofs2)
        continue;
      for (int b = 0; b < bs; ++b)
        active[d * bs + b] = 1;
    }
}

// the population of a mask, added to *count (cleared before the launch): one integer atomic per block
__global__ void __launch_bounds__(PS_THREADS)
k_ml_count(int64_t n, const uint8_t* __restrict__ active, unsigned long long* __restrict__ count)
{
  __shared__ unsigned long long sh[PS_THREADS];
  const int t = threadIdx.x;
  unsigned long long mine = 0;
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + t; d < n; d += (int64_t)gridDim.x * PS_THREADS)
    mine += active[d] ? 1u : 0u;
  sh[t] = mine;
  __syncthreads();
  for (int half = PS_THREADS / 2; half > 0; half >>= 1)
  {
    if (t < half)
      sh[t] += sh[t + half];
    __syncthreads();
  }
  if (t == 0 && sh[0])
    atomicAdd(count, sh[0]);
}

// u += alpha d, r -= alpha q on the free rows; partials of r.r of column k: part[2 k][block]
template <int NC>
__global__ void __launch_bounds__(PS_THREADS)
k_ml_update(int64_t n, const ManyCols cols, const double* __restrict__ p, const double* __restrict__ q,
            const uint8_t* __restrict__ fixed, double* __restrict__ u, double* __restrict__ r, double* __restrict__ part)
{
#pragma clang fp contract(off)
  __shared__ double sh[NC][PS_THREADS];
  const uint32_t live = cols_live<NC>(cols);
  if (!live)
    return;
  const int t = threadIdx.x;
  double alpha[NC], a0[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k)
  {
    alpha[k] = col_on<NC>(live, k) ? cols.st[k].alpha : 0.0;
    a0[k] = 0.0;
  }
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + t; d < n; d += (int64_t)gridDim.x * PS_THREADS)
  {
    if (fixed[d])
      continue; // (r is 0 there since the start)
#pragma unroll
    for (int k = 0; k < NC; ++k)
    {
      if (!col_on<NC>(live, k))
        continue;
      const int64_t e = k * n + d;
      u[e] = u[e] + alpha[k] * p[e];
      const double rv = r[e] - alpha[k] * q[e];
      r[e] = rv;
      a0[k] = a0[k] + rv * rv;
    }
  }
#pragma unroll
  for (int k = 0; k < NC; ++k)
    sh[k][t] = a0[k];
  __syncthreads();
  EQLB_BLOCK_TREE_SUM(sh, t, NC, PS_THREADS)
  if (t < NC && col_on<NC>(live, t))
    part[(int64_t)(2 * t) * gridDim.x + blockIdx.x] = sh[t][0];
}

// partials of x.y of column k: part[2 k + 1][block]
template <int NC>
__global__ void __launch_bounds__(PS_THREADS)
k_ml_dot(int64_t n, const ManyCols cols, const double* __restrict__ x, const double* __restrict__ y,
         double* __restrict__ part)
{
#pragma clang fp contract(off)
  __shared__ double sh[NC][PS_THREADS];
  const uint32_t live = cols_live<NC>(cols);
  if (!live)
    return;
  const int t = threadIdx.x, G = gridDim.x;
  double a0[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k)
    a0[k] = 0.0;
  for (int64_t d = (int64_t)blockIdx.x * PS_THREADS + t; d < n; d += (int64_t)G * PS_THREADS)
  {
#pragma unroll
    for (int k = 0; k < NC; ++k)
      if (col_on<NC>(live, k))
        a0[k] = a0[k] + x[k * n + d] * y[k * n + d];
  }
#pragma unroll
  for (int k = 0; k < NC; ++k)
    sh[k][t] = a0[k];
  __syncthreads();
  EQLB_BLOCK_TREE_SUM(sh, t, NC, PS_THREADS)
  if (t < NC && col_on<NC>(live, t))
    part[(int64_t)(2 * t + 1) * G + blockIdx.x] = sh[t][0];
}
} // namespace
} // namespace eqlb

// the handle behind eqlb_hierarchy_t: views of the borrowed levels and the work space
struct eqlb_hierarchy
{
  struct Vectors // of one level, [R][n_l] each
  {
    double *r, *z, *t;
  };
  int nlevels = 0, bs = 0, p = 0;
  std::vector<eqlb::SolverLevel> lv;
  std::vector<eqlb_refine*> plans;
  std::vector<int64_t> n; // bs * ndofs per level
  eqlb::DevCarve mem;
  std::vector<eqlb::DevPiece<double>> r, z, t; // one column: carved at create
  std::vector<Vectors> one, wide;              // the views for one column, and for wide_R of them: grown on demand
  int wide_R = 0;
  eqlb::DevBuf<char> wide_mem;
  // local smoothing: the masks of the levels l >= 1 (level 0 has none), carved at create and allocated by the first
  // eqlb_hierarchy_set_local(1); their populations
  int local = 0;
  eqlb::DevCarve act_mem;
  std::vector<eqlb::DevPiece<uint8_t>> act;
  eqlb::DevPiece<unsigned long long> act_count_dev; // [nlevels]
  std::vector<int64_t> act_count;
  // the exact solve on level 0: the factor of the last eqlb_hierarchy_set_coarse(1), kept until the handle ends
  eqlb::CoarseSolve coarse;
};

namespace eqlb
{
namespace
{
// What every entry that runs the preconditioner does after its checks, for the R <= MANY_R columns of its groups: the
// work space - r_l, z_l, t_l here, y_loc (and, on the finest level, the vectors of the CG) in the solver handles
int prepare(eqlb_hierarchy* h, int R)
{
  PcgWork w;
  for (int l = 0; l < h->nlevels; ++l)
    EQLB_TRY(h->lv[l].work(h->lv[l].handle, R, w));
  if (R > 1 && R > h->wide_R && h->nlevels > 1)
  {
    std::vector<size_t> off(3 * h->nlevels);
    size_t bytes = 0;
    for (int l = 0; l < h->nlevels; ++l)
      for (int j = 0; j < 3; ++j)
      {
        off[3 * l + j] = bytes;
        bytes += round_up256((size_t)R * h->n[l] * sizeof(double));
      }
    h->wide_R = 0;
    HIP_TRY(h->wide_mem.alloc_raw(bytes)); // (frees the smaller one first)
    h->wide.resize(h->nlevels);
    auto dp = [&](size_t o) { return reinterpret_cast<double*>(h->wide_mem.get() + o); };
    for (int l = 0; l < h->nlevels; ++l)
      h->wide[l] = {dp(off[3 * l]), dp(off[3 * l + 1]), dp(off[3 * l + 2])};
    h->wide_R = R;
  }
  return EQLB_OK;
}

// level + 1 -> level on the columns of c: the store pass into the y_loc of the coarse handle, then its owner sum
int enqueue_restrict(const char* who, const eqlb_hierarchy& h, int level, const ManyCols& c, const double* r_fine,
                     double* r_coarse, bool masked, hipStream_t stream)
{
  const SolverLevel &lo = h.lv[level], &hi = h.lv[level + 1];
  PcgWork w;
  EQLB_TRY(lo.work(lo.handle, c.R, w)); // (grown by prepare: a view)
  EQLB_TRY(launch_restrict(who, h.plans[level], hi.mesh, h.p, h.bs, c, hi.cell_dofs, hi.ndofs, r_fine, w.yloc,
                           stream));
  HIP_TRY(lo.owner_sum(lo.handle, c, r_coarse, masked, stream));
  return EQLB_OK;
}

// z_0 on level 0 from r_0, on the columns of c: the diagonal, or the exact solve (eqlb_coarse.hip)
int enqueue_coarsest(const eqlb_hierarchy& h, const ManyCols& c, const double* r, double* z, hipStream_t stream)
{
  if (h.coarse.on)
  {
    HIP_TRY(coarse_apply(h.coarse, c, r, h.lv[0].fixed, z, stream));
    return EQLB_OK;
  }
  const double* const none = nullptr;
  EQLB_LAUNCH_COLS(MANY_R, k_ml_combine, c.R, h.n[0], stream, h.n[0], c, none, r, h.lv[0].diag, h.lv[0].fixed, z);
  HIP_TRY(hipGetLastError());
  return EQLB_OK;
}

// z = M r on the finest level, on the columns of c; r, z DEVICE [R][n_L]; 2 + 4 L launches whatever R is (3 + 4 L with
// the exact solve on level 0)
int enqueue_precondition(const char* who, const eqlb_hierarchy& h, const ManyCols& c, const double* r, double* z,
                         hipStream_t stream)
{
  const int L = h.nlevels - 1;
  if (L == 0)
    return enqueue_coarsest(h, c, r, z, stream);
  const std::vector<eqlb_hierarchy::Vectors>& v = c.R == 1 ? h.one : h.wide;
  EQLB_LAUNCH_COLS(MANY_R, k_ml_mask, c.R, h.n[L], stream, h.n[L], c, r, h.lv[L].fixed, v[L].r);
  HIP_TRY(hipGetLastError());
  for (int l = L - 1; l >= 0; --l)
    EQLB_TRY(enqueue_restrict(who, h, l, c, v[l + 1].r, v[l].r, true, stream));
  EQLB_TRY(enqueue_coarsest(h, c, v[0].r, v[0].z, stream));
  for (int l = 1; l <= L; ++l)
  {
    // (k_prolong knows no stop flag and no columns to leave out: it prolongs all R, into a t_l whose idle columns
    // nobody reads)
    EQLB_TRY(eqlb_refine_prolong_lagrange(h.plans[l - 1], h.lv[l].mesh, h.p, h.bs, c.R, h.lv[l - 1].cell_dofs,
                                          h.lv[l - 1].ndofs, v[l - 1].z, h.lv[l].cell_dofs, h.lv[l].ndofs, v[l].t,
                                          EQLB_MEM_DEVICE, stream));
    if (h.local)
      EQLB_LAUNCH_COLS(MANY_R, k_ml_combine_local, c.R, h.n[l], stream, h.n[l], c, static_cast<const double*>(v[l].t),
                       static_cast<const double*>(v[l].r), h.lv[l].diag, h.lv[l].fixed,
                       static_cast<const uint8_t*>(h.act[l].get()), l == L ? z : v[l].z);
    else
      EQLB_LAUNCH_COLS(MANY_R, k_ml_combine, c.R, h.n[l], stream, h.n[l], c, static_cast<const double*>(v[l].t),
                       static_cast<const double*>(v[l].r), h.lv[l].diag, h.lv[l].fixed, l == L ? z : v[l].z);
    HIP_TRY(hipGetLastError());
  }
  return EQLB_OK;
}

// the preconditioner inside pcg_solve (eqlb_primal_common.h: JacobiSteps is the counterpart)
struct MultilevelSteps
{
  static constexpr int max_cols = MANY_R;
  static constexpr int check_every = ML_CHECK_EVERY;
  const char* who;
  const eqlb_hierarchy& h;
  const PcgWork& w;
  hipStream_t stream;
  hipError_t rz_and_scalar(const ManyCols& c, int step) const
  {
    EQLB_LAUNCH_COLS(MANY_R, k_ml_dot, w.R, w.n, stream, w.n, c, static_cast<const double*>(w.r),
                     static_cast<const double*>(w.z), w.part);
    return launch_scalar(w, c.mask, step, 1, 0.0, 0.0, nullptr, stream);
  }
  // (the residual launch has left the partials of r.r in channel 0)
  hipError_t restart(const ManyCols& c, int step, double, double) const
  {
    if (enqueue_precondition(who, h, c, w.r, w.z, stream) != EQLB_OK)
      return hipErrorUnknown;
    return rz_and_scalar(c, step);
  }
  hipError_t advance(const ManyCols& c, double* pu, double, double) const
  {
    EQLB_LAUNCH_COLS(MANY_R, k_ml_update, w.R, w.n, stream, w.n, c, static_cast<const double*>(w.d),
                     static_cast<const double*>(w.q), w.fixed, pu, w.r, w.part);
    if (enqueue_precondition(who, h, c, w.r, w.z, stream) != EQLB_OK)
      return hipErrorUnknown;
    return rz_and_scalar(c, STEP_BETA);
  }
};

// what the *_many entries check beyond the single ones (many), and the memory space
int check_columns(const char* who, const eqlb_hierarchy* h, bool many, int32_t nrhs, int32_t memspace)
{
  if (many && nrhs < 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: nrhs = %d (at least 1)", who, (int)nrhs);
  if (many && h->bs != 1)
    return fail(EQLB_ERR_UNSUPPORTED, "%s: several right-hand sides are provided for Poisson handles (bs = 1) only", who);
  return check_memspace(who, memspace);
}

// eqlb_hierarchy_precondition and eqlb_hierarchy_precondition_many behind their names
int hierarchy_precondition(const char* who, bool many, eqlb_hierarchy* h, int32_t nrhs, const double* r, double* z,
                           int32_t memspace, void* stream_)
{
  if (!h || !r || !z)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  EQLB_TRY(check_columns(who, h, many, nrhs, memspace));
  EQLB_TRY(prepare(h, nrhs < MANY_R ? nrhs : MANY_R));
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
    st = enqueue_precondition(who, *h, ManyCols{R, (1u << R) - 1u, 0, nullptr}, pr + c0 * n, pz + c0 * n, stream);
  }
  HIP_TRY(s.finish(stream));
  return st;
}

// eqlb_hierarchy_solve and eqlb_hierarchy_solve_many behind their names
int hierarchy_solve(const char* who, bool many, eqlb_hierarchy* h, int32_t nrhs, const double* b, double* u,
                    double rtol, double atol, int32_t maxit, double* info, int32_t memspace, void* stream_)
{
  if (maxit < 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: maxit = %d (at least 1)", who, (int)maxit);
  if (!(rtol >= 0.0) || !(atol >= 0.0))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: rtol = %g, atol = %g negative or NaN", who, rtol, atol);
  if (!h || !b || !u || !info)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  EQLB_TRY(check_columns(who, h, many, nrhs, memspace));
  EQLB_TRY(prepare(h, nrhs < MANY_R ? nrhs : MANY_R));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const SolverLevel& top = h->lv[h->nlevels - 1];
  // the status word of the finest mask: the call waits by nature, and nothing is launched for a singular problem
  int32_t status[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(status, top.status, sizeof(status), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  for (int c = 0; c < h->bs; ++c)
    if (status[1 + c] < 1 && !top.definite(top.handle))
      return many ? fail(EQLB_ERR_INVALID_ARGUMENT, "%s: singular: the finest level has no Dirichlet DOF", who)
                  : fail(EQLB_ERR_INVALID_ARGUMENT,
                         "%s: singular: component %d of the finest level has no Dirichlet DOF", who, c);
  auto residual = [&](const ManyCols& c, const double* xb, const double* xu, double* r, bool only_fixed) {
    return top.residual(top.handle, c, xb, xu, r, only_fixed, stream);
  };
  auto product = [&](const ManyCols& c) { return top.product(top.handle, c, stream); };
  return pcg_solve_groups(h->n[h->nlevels - 1], nrhs, b, u, info, memspace == EQLB_MEM_HOST, stream,
                          [&](int R, const double* pb, double* pu, double* pinfo) {
                            PcgWork w;
                            EQLB_TRY(top.work(top.handle, R, w)); // (grown by prepare: a view)
                            return pcg_solve(w, residual, product, MultilevelSteps{who, *h, w, stream}, pb, pu, rtol,
                                             atol, maxit, pinfo, status[0], stream);
                          });
}
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
  h->one.resize(nlevels);
  for (int l = 0; l < nlevels; ++l)
    h->one[l] = {h->r[l].get(), h->z[l].get(), h->t[l].get()};
  h->act.resize(nlevels);
  for (int l = 1; l < nlevels; ++l)
    h->act[l] = h->act_mem.piece<uint8_t>((size_t)h->n[l]);
  h->act_count_dev = h->act_mem.piece<unsigned long long>((size_t)nlevels);
  h->act_count.assign(nlevels, 0);
  *out = h.release();
  return EQLB_OK;
}
EQLB_CATCH_ALL

void eqlb_hierarchy_destroy(eqlb_hierarchy_t* handle) { delete handle; }

int eqlb_hierarchy_set_local(eqlb_hierarchy_t* h, int32_t local, void* stream_)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_hierarchy_set_local";
  if (!h)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  if (local != 0 && local != 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: local = %d is not 0 or 1", who, (int)local);
  if (local == h->local)
    return EQLB_OK;
  if (local == 0)
  {
    h->local = 0;
    return EQLB_OK;
  }
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!h->act_mem.base())
    HIP_TRY(h->act_mem.alloc());
  // (the masks follow from the plans alone, but they are written again on the stream of this call: what runs behind it
  // on that stream finds them)
  HIP_TRY(hipMemsetAsync(h->act_mem.base(), 0, h->act_mem.bytes(), stream));
  const int nd = nd_of(h->p);
  for (int l = 1; l < h->nlevels; ++l)
  {
    const eqlb_refine& pl = *h->plans[l - 1];
    hipLaunchKernelGGL(k_ml_active, dim3(grid_of(pl.ncells, PS_THREADS)), dim3(PS_THREADS), 0, stream, pl.ncells,
                       (int64_t)pl.ncells2, static_cast<const uint32_t*>(pl.coff.get()), nd, h->bs, h->lv[l].cell_dofs,
                       h->lv[l].ndofs, h->act[l].get());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_ml_count, dim3(stream_blocks(h->n[l])), dim3(PS_THREADS), 0, stream, h->n[l],
                       static_cast<const uint8_t*>(h->act[l].get()), h->act_count_dev.get() + l);
    HIP_TRY(hipGetLastError());
  }
  std::vector<unsigned long long> cnt(h->nlevels, 0);
  HIP_TRY(hipMemcpyAsync(cnt.data(), h->act_count_dev.get(), cnt.size() * sizeof(cnt[0]), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  for (int l = 1; l < h->nlevels; ++l)
    h->act_count[l] = (int64_t)cnt[l];
  h->act_count[0] = h->n[0];
  h->local = 1;
  return EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_hierarchy_set_coarse(eqlb_hierarchy_t* h, int32_t coarse, void* stream_)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_hierarchy_set_coarse";
  if (!h)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  if (coarse != 0 && coarse != 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: coarse = %d is not 0 or 1", who, (int)coarse);
  if (coarse == 0)
  {
    h->coarse.on = 0; // (the factor keeps its memory)
    return EQLB_OK;
  }
  // (every call factors again: the factor is a snapshot of the mask and the coefficient of level 0)
  return coarse_setup(who, h->coarse, h->lv[0], reinterpret_cast<hipStream_t>(stream_));
}
EQLB_CATCH_ALL

int eqlb_hierarchy_coarse_rows(eqlb_hierarchy_t* h, int64_t* n)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_hierarchy_coarse_rows";
  if (!h || !n)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  if (!h->coarse.on)
    return fail(EQLB_ERR_INVALID_ARGUMENT,
                "%s: level 0 is treated by its diagonal: switch the exact solve on first (eqlb_hierarchy_set_coarse)", who);
  *n = h->coarse.n;
  return EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_hierarchy_coarse_factor(eqlb_hierarchy_t* h, int32_t* rows, double* d, double* W, int64_t capacity,
                                 int32_t memspace, void* stream_)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_hierarchy_coarse_factor";
  if (!h || !rows || !d || !W)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  if (!h->coarse.on)
    return fail(EQLB_ERR_INVALID_ARGUMENT,
                "%s: level 0 is treated by its diagonal: switch the exact solve on first (eqlb_hierarchy_set_coarse)", who);
  EQLB_TRY(check_memspace(who, memspace));
  const size_t n = (size_t)h->coarse.n;
  if (capacity < (int64_t)n)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: capacity = %lld below the %lld free rows of level 0", who,
                (long long)capacity, (long long)n);
  if (n == 0)
    return EQLB_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const hipMemcpyKind kind = memspace == EQLB_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  HIP_TRY(hipMemcpyAsync(rows, h->coarse.rows.get(), n * sizeof(int32_t), kind, stream));
  HIP_TRY(hipMemcpyAsync(d, h->coarse.d.get(), n * sizeof(double), kind, stream));
  HIP_TRY(hipMemcpyAsync(W, h->coarse.W.get(), n * n * sizeof(double), kind, stream));
  if (memspace == EQLB_MEM_HOST)
    HIP_TRY(hipStreamSynchronize(stream));
  return EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_hierarchy_active(eqlb_hierarchy_t* h, int32_t level, uint8_t* out, int64_t capacity, int32_t memspace,
                          void* stream_)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_hierarchy_active";
  if (!h || !out)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  if (!h->local)
    return fail(EQLB_ERR_INVALID_ARGUMENT,
                "%s: the hierarchy smooths every row: switch local smoothing on first (eqlb_hierarchy_set_local)", who);
  if (level < 0 || level > h->nlevels - 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: level = %d outside 0 ... %d", who, (int)level, h->nlevels - 1);
  EQLB_TRY(check_memspace(who, memspace));
  const int64_t n = h->n[level];
  if (capacity < n)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: capacity = %lld below the %lld rows of level %d", who,
                (long long)capacity, (long long)n, (int)level);
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (memspace == EQLB_MEM_DEVICE)
  {
    if (level == 0)
      HIP_TRY(hipMemsetAsync(out, 1, (size_t)n, stream));
    else
      HIP_TRY(hipMemcpyAsync(out, h->act[level].get(), (size_t)n, hipMemcpyDeviceToDevice, stream));
    return EQLB_OK;
  }
  if (level == 0)
  {
    std::fill(out, out + n, (uint8_t)1);
    return EQLB_OK;
  }
  HIP_TRY(hipMemcpyAsync(out, h->act[level].get(), (size_t)n, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_hierarchy_active_count(eqlb_hierarchy_t* h, int32_t level, int64_t* count)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_hierarchy_active_count";
  if (!h || !count)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  if (!h->local)
    return fail(EQLB_ERR_INVALID_ARGUMENT,
                "%s: the hierarchy smooths every row: switch local smoothing on first (eqlb_hierarchy_set_local)", who);
  if (level < 0 || level > h->nlevels - 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: level = %d outside 0 ... %d", who, (int)level, h->nlevels - 1);
  *count = h->act_count[level];
  return EQLB_OK;
}
EQLB_CATCH_ALL

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
  const int st = enqueue_restrict(who, *h, level, ManyCols{1, 1u, 0, nullptr}, host ? d_in.get() : r_fine,
                                  host ? d_out.get() : r_coarse, masked != 0, stream);
  HIP_TRY(s.finish(stream));
  return st;
}
EQLB_CATCH_ALL

int eqlb_hierarchy_precondition(eqlb_hierarchy_t* h, const double* r, double* z, int32_t memspace, void* stream_)
try
{
  return eqlb::hierarchy_precondition("eqlb_hierarchy_precondition", false, h, 1, r, z, memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_hierarchy_precondition_many(eqlb_hierarchy_t* h, int32_t nrhs, const double* r, double* z, int32_t memspace,
                                     void* stream_)
try
{
  return eqlb::hierarchy_precondition("eqlb_hierarchy_precondition_many", true, h, nrhs, r, z, memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_hierarchy_solve(eqlb_hierarchy_t* h, const double* b, double* u, double rtol, double atol, int32_t maxit,
                         double* info, int32_t memspace, void* stream_)
try
{
  return eqlb::hierarchy_solve("eqlb_hierarchy_solve", false, h, 1, b, u, rtol, atol, maxit, info, memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_hierarchy_solve_many(eqlb_hierarchy_t* h, int32_t nrhs, const double* b, double* u, double rtol, double atol,
                              int32_t maxit, double* info, int32_t memspace, void* stream_)
try
{
  return eqlb::hierarchy_solve("eqlb_hierarchy_solve_many", true, h, nrhs, b, u, rtol, atol, maxit, info, memspace,
                               stream_);
}
EQLB_CATCH_ALL

} // extern "C"
