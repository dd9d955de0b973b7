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
// This unit holds the cell kernel, its dispatch on p, d and R, the table getters and the C entries.  The sum pass, the
// mask, the CG kernels and the host loop lie in eqlb_primal_common.h; the handle, the launches on it and the bodies of the
// C entries in eqlb_primal_handle.h.  eqlb_primal_elasticity.hip shares both.
// Several right-hand sides in one call (eqlb_primal_apply_many, eqlb_primal_solve_many) run on the same kernels and
// the same host loop: k_primal_cell<P, CELL_OPERATOR, 0, R> here, the rest in eqlb_primal_common.h, which states the
// rule.  The work space for one column is carved at create, the one for more is grown on demand (primal_work).
#include "eqlb_device_common.h"
#include "eqlb_primal_handle.h" // the host side of a solver handle; eqlb_primal_common.h: the kernels it launches
#include "eqlb_tables_gen.h"

#include <cmath>

// the handle behind eqlb_primal_t
struct eqlb_primal : eqlb::SolverHandle<1, eqlb::MANY_R>
{
};

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

// the hook of eqlb_primal_handle.h, the store pass on the columns of c: u [R][ndofs] (load: rhs_dg) into the y_loc of the
// work space for c.R columns
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
} // namespace

void primal_level(eqlb_primal* h, SolverLevel& v) { solver_level(h, v); }
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
  return eqlb::solver_create("eqlb_primal_create", std::make_unique<eqlb_primal>(), mesh, p, cell_coeff, memspace,
                             stream_, handle);
}
EQLB_CATCH_ALL

void eqlb_primal_destroy(eqlb_primal_t* handle) { delete handle; }

int eqlb_primal_ndofs(const eqlb_primal_t* handle, int64_t* ndofs)
{
  return eqlb::solver_ndofs("eqlb_primal_ndofs", handle, ndofs);
}

int eqlb_primal_set_dirichlet(eqlb_primal_t* h, int32_t nlist, const int32_t* facets, int32_t memspace, void* stream_)
try
{
  const int32_t nlists[1] = {nlist};
  const int32_t* const lists[1] = {facets};
  return eqlb::solver_set_dirichlet("eqlb_primal_set_dirichlet", h, nlists, lists, memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_primal_load(eqlb_primal_t* h, int32_t degree_dg, const double* rhs_dg, const double* b_extra, double* b,
                     int32_t memspace, void* stream_)
try
{
  return eqlb::solver_load("eqlb_primal_load", h, degree_dg, rhs_dg, b_extra, b, memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_primal_apply(eqlb_primal_t* h, const double* u, double* y, int32_t masked, int32_t memspace, void* stream_)
try
{
  return eqlb::solver_apply("eqlb_primal_apply", h, 1, u, y, masked, memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_primal_apply_many(eqlb_primal_t* h, int32_t nrhs, const double* u, double* y, int32_t masked,
                           int32_t memspace, void* stream_)
try
{
  return eqlb::solver_apply("eqlb_primal_apply_many", h, nrhs, u, y, masked, memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_primal_diagonal(eqlb_primal_t* h, double* out, int32_t memspace, void* stream_)
try
{
  return eqlb::solver_diagonal("eqlb_primal_diagonal", h, out, memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_primal_residual(eqlb_primal_t* h, const double* b, const double* u, double* r, double* norms,
                         int32_t memspace, void* stream_)
try
{
  return eqlb::solver_residual("eqlb_primal_residual", h, b, u, r, norms, memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_primal_solve(eqlb_primal_t* h, const double* b, double* u, double rtol, double atol, int32_t maxit,
                      double* info, int32_t memspace, void* stream_)
try
{
  return eqlb::solver_solve("eqlb_primal_solve", h, 1, b, u, rtol, atol, maxit, info, memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_primal_solve_many(eqlb_primal_t* h, int32_t nrhs, const double* b, double* u, double rtol, double atol,
                           int32_t maxit, double* info, int32_t memspace, void* stream_)
try
{
  return eqlb::solver_solve("eqlb_primal_solve_many", h, nrhs, b, u, rtol, atol, maxit, info, memspace, stream_);
}
EQLB_CATCH_ALL

} // extern "C"
