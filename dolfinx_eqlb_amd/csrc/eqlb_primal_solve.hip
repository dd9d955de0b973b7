// The P_p Poisson problem -div(kappa grad u) = f ON THE DEVICE: the operator applied matrix-free on the handle's own
// P_p space (the numbering of eqlb_mesh_lagrange_dofmap), the load vector from DG_d data, the residual of a given u_h
// and a Jacobi-preconditioned CG - the primal solves of the reference's adaptive demos (demo/poisson_adaptive/
// demo_lshape.py, demo_discont-coeff.py, demo/poisson/demo_reconstruction.py), which no DOLFINx can do on a mesh that
// was refined on the device.  The rule is stated in include/eqlb.h and, as numpy, in dolfinx_eqlb_amd/lsolver/primal.py;
// operator, load, diagonal and residual reproduce the numpy statement bit for bit.
//
// The operator is a store pass plus a per-destination sum pass - no atomics, one fixed order of operations per value:
//  k_primal_cell<P, MODE, D, R>  one thread per cell, PS_THREADS cells per workgroup.  The table (Stiff<P>: 675 doubles,
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
// The sum pass, the CG kernels and the host loop lie in eqlb_primal_common.h, which eqlb_primal_elasticity.hip shares.
// Several right-hand sides in one call (eqlb_primal_apply_many, eqlb_primal_solve_many) run on the same kernels and
// the same host loop: k_primal_cell<P, CELL_OPERATOR, 0, R> here, the rest in eqlb_primal_common.h, which states the
// rule.  The work space for one column is carved at create, the one for more is grown on demand (primal_work).
#include "eqlb_device_common.h"
#include "eqlb_mesh_handle.h" // (eqlb_host_util.h)
#include "eqlb_primal_common.h" // the sum pass, the kernels and the host loop of the CG: shared with the elasticity unit
#include "eqlb_tables_gen.h"

#include <climits>
#include <cmath>

namespace eqlb
{
namespace
{
struct CellArgs
{
  int32_t ncells;
  const int32_t* cell_dofs; // [ncells][nd_p]
  const double *cellJ, *coeff;
  const double* u;      // operator: column 0 of [R][ndofs], column c at u + c * ustride; load: rhs_dg [ncells][nd_d]
  const uint8_t* fixed; // operator, only_fixed: the free rows of u read as 0
  int32_t only_fixed;
  double* yloc; // [ncells][nd_p], column c at yloc + c * ystride
};

// MODE = CELL_OPERATOR runs on R columns: the index row, J, the coefficient and the table are read once and applied to
// the columns of u.  A table entry is read from LDS once and multiplied into the R sums, each of which runs in the one
// order.  With R > 1 the R rows of a cell stay in registers (R nd_p solution values, R nd_p results) and go out column
// by column through the one sbuf, so the LDS footprint does not depend on R; with R = 1 the row goes straight to sbuf.
// Columns that do not run (ManyCols) are neither read nor written.  Diagonal and load know one column.
template <int P, int MODE, int D, int R>
__global__ void __launch_bounds__(PS_THREADS) k_primal_cell(const CellArgs a, const ManyCols cols, int64_t ustride,
                                                            int64_t ystride)
{
#pragma clang fp contract(off) // the statement rounds every product and every sum on its own
  constexpr int NP = nd_of(P), ND = nd_of(D), S = NP | 1;
  constexpr int NTAB = (MODE == CELL_LOAD) ? NP * ND : 3 * NP * NP;
  static_assert(eqlb_tables::Stiff<P>::ND == NP && eqlb_tables::Load<P, D>::NP == NP && eqlb_tables::Load<P, D>::ND == ND,
                "table shape");
  static_assert(R >= 1 && R <= MANY_R && (R == 1 || MODE == CELL_OPERATOR), "columns for the operator only");
  __shared__ double sT[NTAB];
  __shared__ double sbuf[PS_THREADS * S]; // first the index rows of the workgroup, then its output rows, a column at a time
  const uint32_t live = cols_live<R>(cols);
  if (!live)
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
  [[maybe_unused]] double out[R > 1 ? R : 1][R > 1 ? NP : 1];
  if constexpr (R > 1)
  {
#pragma unroll
    for (int c = 0; c < R; ++c)
#pragma unroll
      for (int i = 0; i < NP; ++i)
        out[c][i] = 0.0;
  }
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
      [[maybe_unused]] double uu[R][NP];
      if constexpr (MODE == CELL_OPERATOR)
      {
#pragma unroll
        for (int i = 0; i < NP; ++i)
        {
          const bool zero = a.only_fixed && !a.fixed[idx[i]];
#pragma unroll
          for (int c = 0; c < R; ++c)
          {
            const double v = col_on<R>(live, c) ? a.u[c * ustride + idx[i]] : 0.0;
            uu[c][i] = zero ? 0.0 : v;
          }
        }
      }
#pragma unroll
      for (int i = 0; i < NP; ++i)
      {
        double tm[R][3];
#pragma unroll
        for (int m = 0; m < 3; ++m)
        {
          const double* row = sT + (m * NP + i) * NP;
          if constexpr (MODE == CELL_DIAGONAL)
            tm[0][m] = row[i];
          else
          {
            double s[R];
            {
              const double e = row[0];
#pragma unroll
              for (int c = 0; c < R; ++c)
                s[c] = e * uu[c][0];
            }
#pragma unroll
            for (int j = 1; j < NP; ++j)
            {
              const double e = row[j];
#pragma unroll
              for (int c = 0; c < R; ++c)
                s[c] = s[c] + e * uu[c][j];
            }
#pragma unroll
            for (int c = 0; c < R; ++c)
              tm[c][m] = s[c];
          }
        }
#pragma unroll
        for (int c = 0; c < R; ++c)
        {
          const double v = w * ((C00 * tm[c][0] + C01 * tm[c][1]) + C11 * tm[c][2]);
          if constexpr (R == 1)
            sbuf[t * S + i] = v;
          else
            out[c][i] = v;
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < R; ++c)
  {
    if (!col_on<R>(live, c)) // (the same in every thread)
      continue;
    if constexpr (R > 1)
    {
      if (active)
      {
#pragma unroll
        for (int i = 0; i < NP; ++i)
          sbuf[t * S + i] = out[c][i];
      }
    }
    __syncthreads();
    double* o = a.yloc + c * ystride + base * NP;
    for (int e = t; e < nloc * NP; e += PS_THREADS)
      o[e] = sbuf[(e / NP) * S + (e % NP)];
    if constexpr (R > 1)
      __syncthreads(); // (the next column overwrites sbuf)
  }
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


// ---- host side ------------------------------------------------------------------------------------------------
// the launch on the columns of c: the load by its DG degree d, the operator by its column count, the diagonal as it is
template <int P, int MODE>
hipError_t launch_cell_p(int d, const CellArgs& a, const ManyCols& c, int64_t ustride, int64_t ystride,
                         hipStream_t stream)
{
  const dim3 grid(grid_of(a.ncells, PS_THREADS)), block(PS_THREADS);
#define EQLB_CELL(DD, RR)                                                                                              \
  hipLaunchKernelGGL((k_primal_cell<P, MODE, DD, RR>), grid, block, 0, stream, a, c, ustride, ystride)
  if constexpr (MODE == CELL_LOAD)
    switch (d)
    {
    case 0:
      EQLB_CELL(0, 1);
      break;
    case 1:
      EQLB_CELL(1, 1);
      break;
    case 2:
      EQLB_CELL(2, 1);
      break;
    default:
      EQLB_CELL(3, 1);
    }
  else if constexpr (MODE == CELL_OPERATOR)
    switch (c.R)
    {
    case 1:
      EQLB_CELL(0, 1);
      break;
    case 2:
      EQLB_CELL(0, 2);
      break;
    case 3:
      EQLB_CELL(0, 3);
      break;
    default:
      EQLB_CELL(0, 4);
    }
  else
    EQLB_CELL(0, 1);
#undef EQLB_CELL
  return hipGetLastError();
}

template <int MODE>
hipError_t launch_cell(int p, int d, const CellArgs& a, const ManyCols& c, int64_t ustride, int64_t ystride,
                       hipStream_t stream)
{
  switch (p)
  {
  case 1:
    return launch_cell_p<1, MODE>(d, a, c, ustride, ystride, stream);
  case 2:
    return launch_cell_p<2, MODE>(d, a, c, ustride, ystride, stream);
  case 3:
    return launch_cell_p<3, MODE>(d, a, c, ustride, ystride, stream);
  default:
    return launch_cell_p<4, MODE>(d, a, c, ustride, ystride, stream);
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
  // the work space for 2 ... MANY_R columns (wide.R of them): grown by the first call that needs it, then reused
  eqlb::DevBuf<char> wide_mem;
  eqlb::PcgWork wide{};
};

namespace eqlb
{
namespace
{
const ManyCols ONE_COLUMN{1, 1u, 0, nullptr}; // a launch on one vector that knows no state

// the work space the launches on R columns use: the carve of the handle for one, the grown one (primal_work) for more
PcgWork work_of(const eqlb_primal& h, int R)
{
  PcgWork w = R == 1 ? PcgWork{h.ndofs, 1, h.diag, h.fixed, h.yloc, h.r, h.z, h.d, h.q, h.part, h.st} : h.wide;
  w.R = R;
  return w;
}

// grows the work space for R > 1 columns if need be
int primal_work(eqlb_primal* h, int R, PcgWork& w)
{
  if (R > 1 && R > h->wide.R)
  {
    const size_t n = (size_t)h->ndofs, ny = (size_t)h->space.ncells * h->nd;
    size_t off = 0;
    auto piece = [&](size_t bytes) {
      const size_t o = off;
      off += round_up256(bytes);
      return o;
    };
    const size_t o_y = piece(R * ny * sizeof(double)), o_r = piece(R * n * sizeof(double)),
                 o_z = piece(R * n * sizeof(double)), o_d = piece(R * n * sizeof(double)),
                 o_q = piece(R * n * sizeof(double)), o_p = piece((size_t)R * 2 * PS_MAXBLOCKS * sizeof(double)),
                 o_s = piece(R * sizeof(PcgState));
    h->wide = PcgWork{};
    HIP_TRY(h->wide_mem.alloc_raw(off)); // (frees the smaller one first)
    char* base = h->wide_mem.get();
    auto dp = [&](size_t o) { return reinterpret_cast<double*>(base + o); };
    h->wide = PcgWork{h->ndofs, R,        h->diag,  h->fixed, dp(o_y), dp(o_r),
                      dp(o_z),  dp(o_d),  dp(o_q),  dp(o_p),  reinterpret_cast<PcgState*>(base + o_s)};
  }
  w = work_of(*h, R);
  return EQLB_OK;
}

// the store pass on the columns of c: u [R][ndofs] (load: rhs_dg) into the y_loc of the work space for c.R columns
template <int MODE>
hipError_t launch_cell(const eqlb_primal& h, const ManyCols& c, int d, const double* u, bool only_fixed,
                       hipStream_t stream)
{
  CellArgs a{};
  a.ncells = h.space.ncells;
  a.cell_dofs = h.cell_dofs;
  a.cellJ = h.mesh->m.cellJ;
  a.coeff = h.has_coeff ? h.coeff.get() : nullptr;
  a.u = u;
  a.fixed = h.fixed;
  a.only_fixed = only_fixed ? 1 : 0;
  a.yloc = work_of(h, c.R).yloc;
  return launch_cell<MODE>(h.p, d, a, c, h.ndofs, (int64_t)h.space.ncells * h.nd, stream);
}

GatherArgs gather_args(const eqlb_primal& h, const ManyCols& c, bool masked)
{
  const PcgWork w = work_of(h, c.R);
  GatherArgs g{};
  g.s = h.space;
  g.yloc = w.yloc;
  g.fixed = masked ? h.fixed.get() : nullptr;
  g.part = w.part;
  g.cols = c;
  g.ystride = (int64_t)h.space.ncells * h.nd;
  return g;
}

hipError_t launch_gather(const eqlb_primal& h, const GatherArgs& g, hipStream_t stream)
{
  const dim3 grid(stream_blocks(h.ndofs)), block(PS_THREADS);
  if (g.cols.R == 1)
    hipLaunchKernelGGL((k_primal_gather<1, 1>), grid, block, 0, stream, g);
  else
    hipLaunchKernelGGL((k_primal_gather<1, MANY_R>), grid, block, 0, stream, g);
  return hipGetLastError();
}

// y = owner sum of y_loc (masked or raw) on the columns of c; y DEVICE [R][ndofs]
hipError_t enqueue_owner_sum(const eqlb_primal& h, const ManyCols& c, double* y, bool masked, hipStream_t stream)
{
  GatherArgs g = gather_args(h, c, masked);
  g.y = y;
  return launch_gather(h, g, stream);
}

hipError_t enqueue_diagonal(const eqlb_primal& h, double* out, hipStream_t stream)
{
  const hipError_t e = launch_cell<CELL_DIAGONAL>(h, ONE_COLUMN, 0, nullptr, false, stream);
  return e != hipSuccess ? e : enqueue_owner_sum(h, ONE_COLUMN, out, false, stream);
}

// r = b - A u (0 on the fixed rows), u^ instead of u with only_fixed; the block partials of r.r are left in part
hipError_t enqueue_residual(const eqlb_primal& h, const ManyCols& c, const double* b, const double* u, double* r,
                            bool only_fixed, hipStream_t stream)
{
  const hipError_t e = launch_cell<CELL_OPERATOR>(h, c, 0, u, only_fixed, stream);
  if (e != hipSuccess)
    return e;
  GatherArgs g = gather_args(h, c, true);
  g.b = b;
  g.r = r;
  g.dot = DOT_R_R;
  return launch_gather(h, g, stream);
}

// q = A d on the free rows (the direction d of the work space), the block partials of d.q in part
hipError_t enqueue_product(const eqlb_primal& h, const ManyCols& c, hipStream_t stream)
{
  const PcgWork w = work_of(h, c.R);
  const hipError_t e = launch_cell<CELL_OPERATOR>(h, c, 0, w.d, false, stream);
  if (e != hipSuccess)
    return e;
  GatherArgs g = gather_args(h, c, true);
  g.y = w.q;
  g.w = w.d;
  g.dot = DOT_W_Y;
  return launch_gather(h, g, stream);
}

int check_handle(const char* who, const eqlb_primal* h)
{
  if (!h)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null handle", who);
  return EQLB_OK;
}

// what every *_many entry checks about its column count
int check_nrhs(const char* who, int32_t nrhs)
{
  if (nrhs < 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: nrhs = %d (at least 1)", who, (int)nrhs);
  return EQLB_OK;
}

// eqlb_primal_apply and eqlb_primal_apply_many behind their names
int primal_apply(const char* who, eqlb_primal* h, int32_t nrhs, const double* u, double* y, int32_t masked,
                 int32_t memspace, void* stream_)
{
  EQLB_TRY(check_handle(who, h));
  EQLB_TRY(check_nrhs(who, nrhs));
  if (!u || !y)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  EQLB_TRY(check_memspace(who, memspace));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool host = memspace == EQLB_MEM_HOST;
  const size_t n = (size_t)h->ndofs;
  PcgWork w;
  EQLB_TRY(primal_work(h, nrhs < MANY_R ? nrhs : MANY_R, w));
  HostCall s;
  const auto d_u = s.in(host ? u : nullptr, nrhs * n);
  const auto d_y = s.out(host ? y : nullptr, nrhs * n);
  if (host)
    HIP_TRY(s.upload(stream));
  const double* pu = host ? d_u.get() : u;
  double* py = host ? d_y.get() : y;
  for (int32_t c0 = 0; c0 < nrhs; c0 += MANY_R)
  {
    const int R = nrhs - c0 < MANY_R ? nrhs - c0 : MANY_R;
    const ManyCols cols{R, (1u << R) - 1u, 0, nullptr};
    s.note(launch_cell<CELL_OPERATOR>(*h, cols, 0, pu + c0 * n, false, stream));
    s.note(enqueue_owner_sum(*h, cols, py + c0 * n, masked != 0, stream));
  }
  HIP_TRY(s.finish(stream));
  return EQLB_OK;
}

// eqlb_primal_solve and eqlb_primal_solve_many behind their names
int primal_solve(const char* who, eqlb_primal* h, int32_t nrhs, const double* b, double* u, double rtol, double atol,
                 int32_t maxit, double* info, int32_t memspace, void* stream_)
{
  if (maxit < 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: maxit = %d (at least 1)", who, (int)maxit);
  if (!(rtol >= 0.0) || !(atol >= 0.0))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: rtol = %g, atol = %g negative or NaN", who, rtol, atol);
  EQLB_TRY(check_handle(who, h));
  EQLB_TRY(check_nrhs(who, nrhs));
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
  PcgWork grown;
  EQLB_TRY(primal_work(h, nrhs < MANY_R ? nrhs : MANY_R, grown));
  auto residual = [&](const ManyCols& c, const double* xb, const double* xu, double* r, bool only_fixed) {
    return enqueue_residual(*h, c, xb, xu, r, only_fixed, stream);
  };
  auto product = [&](const ManyCols& c) { return enqueue_product(*h, c, stream); };
  return pcg_solve_groups(h->ndofs, nrhs, b, u, info, memspace == EQLB_MEM_HOST, stream,
                          [&](int R, const double* pb, double* pu, double* pinfo) {
                            const PcgWork w = work_of(*h, R);
                            return pcg_solve(w, residual, product, JacobiSteps<MANY_R>{w, stream}, pb, pu, rtol, atol, maxit,
                                             pinfo, status[0], stream);
                          });
}
} // namespace

// the handle as the hierarchy unit sees it (eqlb_internal.h: SolverLevel)
void primal_level(eqlb_primal* h, SolverLevel& v)
{
  v = SolverLevel{};
  v.handle = h;
  v.mesh = h->mesh;
  v.p = h->p;
  v.bs = 1;
  v.ndofs = h->ndofs;
  v.cell_dofs = h->cell_dofs;
  v.diag = h->diag;
  v.fixed = h->fixed;
  v.status = h->status;
  v.work = [](void* hh, int R, PcgWork& w) { return primal_work(static_cast<eqlb_primal*>(hh), R, w); };
  v.owner_sum = [](void* hh, const ManyCols& c, double* y, bool masked, hipStream_t stream) {
    return enqueue_owner_sum(*static_cast<eqlb_primal*>(hh), c, y, masked, stream);
  };
  v.residual = [](void* hh, const ManyCols& c, const double* b, const double* u, double* r, bool only_fixed,
                  hipStream_t stream) {
    return enqueue_residual(*static_cast<eqlb_primal*>(hh), c, b, u, r, only_fixed, stream);
  };
  v.product = [](void* hh, const ManyCols& c, hipStream_t stream) {
    return enqueue_product(*static_cast<eqlb_primal*>(hh), c, stream);
  };
}
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
  s.note(launch_cell<CELL_LOAD>(*h, ONE_COLUMN, degree_dg, host ? d_f.get() : rhs_dg, false, stream));
  GatherArgs g = gather_args(*h, ONE_COLUMN, false);
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
  return eqlb::primal_apply("eqlb_primal_apply", h, 1, u, y, masked, memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_primal_apply_many(eqlb_primal_t* h, int32_t nrhs, const double* u, double* y, int32_t masked,
                           int32_t memspace, void* stream_)
try
{
  return eqlb::primal_apply("eqlb_primal_apply_many", h, nrhs, u, y, masked, memspace, stream_);
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
    s.note(enqueue_residual(*h, ONE_COLUMN, pb, pu, h->q, true, stream));
    s.note(launch_scalar(work_of(*h, 1), 1u, STEP_NORM, 0, 0.0, 0.0, pn + 1, stream));
  }
  s.note(enqueue_residual(*h, ONE_COLUMN, pb, pu, host ? d_r.get() : r, false, stream));
  if (pn)
    s.note(launch_scalar(work_of(*h, 1), 1u, STEP_NORM, 0, 0.0, 0.0, pn, stream));
  HIP_TRY(s.finish(stream));
  return EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_primal_solve(eqlb_primal_t* h, const double* b, double* u, double rtol, double atol, int32_t maxit,
                      double* info, int32_t memspace, void* stream_)
try
{
  return eqlb::primal_solve("eqlb_primal_solve", h, 1, b, u, rtol, atol, maxit, info, memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_primal_solve_many(eqlb_primal_t* h, int32_t nrhs, const double* b, double* u, double rtol, double atol,
                           int32_t maxit, double* info, int32_t memspace, void* stream_)
try
{
  return eqlb::primal_solve("eqlb_primal_solve_many", h, nrhs, b, u, rtol, atol, maxit, info, memspace, stream_);
}
EQLB_CATCH_ALL

} // extern "C"
