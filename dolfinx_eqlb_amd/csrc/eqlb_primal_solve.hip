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
// RX adds the reaction term (include/eqlb.h): Mass<P> is staged behind the stiffness tables, an entry is read once and
// multiplied into the R sums as the stiffness entries are, and wm m[i] (diagonal: wm Mass[i][i]) is added to the value
// formed without the term.  The reaction variant is a kernel of its own, k_primal_cell_react, from the same source
// (eqlb_primal_cell.inc), so that a handle without the term launches the instantiations - symbols, arguments and code -
// it launched before the term existed.
// DX replaces the metric K K^T of a cell by K D K^T with the symmetric tensor D_T of eqlb_primal_set_diffusion (include/
// eqlb.h): eight products and four sums more per cell and nothing more per table entry.  Again kernels of their own,
// k_primal_cell_diff and k_primal_cell_diff_react, with an argument the others do not take.
#define EQLB_CELL_DIFF 0
#define EQLB_CELL_REACT 0
#include "eqlb_primal_cell.inc"
#undef EQLB_CELL_REACT
#define EQLB_CELL_REACT 1
#include "eqlb_primal_cell.inc"
#undef EQLB_CELL_REACT
#undef EQLB_CELL_DIFF
#define EQLB_CELL_DIFF 1
#define EQLB_CELL_REACT 0
#include "eqlb_primal_cell.inc"
#undef EQLB_CELL_REACT
#define EQLB_CELL_REACT 1
#include "eqlb_primal_cell.inc"
#undef EQLB_CELL_REACT
#undef EQLB_CELL_DIFF

// ---- host side ------------------------------------------------------------------------------------------------
// the launch on the columns of c: the load by its DG degree d, the operator by its column count, the diagonal as it is
template <int P, int MODE>
hipError_t launch_cell_p(int d, const CellArgs& a, const ManyCols& c, int64_t ustride, int64_t ystride,
                         const ReactArgs* rx, const DiffArgs* dx, hipStream_t stream)
{
  const dim3 grid(grid_of(a.ncells, PS_THREADS)), block(PS_THREADS);
  if constexpr (MODE != CELL_LOAD)
    if (dx) // the variants with the tensor, with the reaction term or without it
    {
#define EQLB_CELL_DX(RR)                                                                                               \
  do                                                                                                                   \
  {                                                                                                                    \
    if (rx)                                                                                                            \
      hipLaunchKernelGGL((k_primal_cell_diff_react<P, MODE, 0, RR>), grid, block, 0, stream, a, c, ustride, ystride,  \
                         *rx, *dx);                                                                                    \
    else                                                                                                               \
      hipLaunchKernelGGL((k_primal_cell_diff<P, MODE, 0, RR>), grid, block, 0, stream, a, c, ustride, ystride, *dx);  \
  } while (0)
      if constexpr (MODE == CELL_DIAGONAL)
        EQLB_CELL_DX(1);
      else
        switch (c.R)
        {
        case 1:
          EQLB_CELL_DX(1);
          break;
        case 2:
          EQLB_CELL_DX(2);
          break;
        case 3:
          EQLB_CELL_DX(3);
          break;
        default:
          EQLB_CELL_DX(4);
        }
#undef EQLB_CELL_DX
      return hipGetLastError();
    }
  if constexpr (MODE != CELL_LOAD)
    if (rx) // the variants with the reaction term; without it the launches below, as before the term existed
    {
#define EQLB_CELL_RX(RR)                                                                                               \
  hipLaunchKernelGGL((k_primal_cell_react<P, MODE, 0, RR>), grid, block, 0, stream, a, c, ustride, ystride, *rx)
      if constexpr (MODE == CELL_DIAGONAL)
        EQLB_CELL_RX(1);
      else
        switch (c.R)
        {
        case 1:
          EQLB_CELL_RX(1);
          break;
        case 2:
          EQLB_CELL_RX(2);
          break;
        case 3:
          EQLB_CELL_RX(3);
          break;
        default:
          EQLB_CELL_RX(4);
        }
#undef EQLB_CELL_RX
      return hipGetLastError();
    }
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
                       const ReactArgs* rx, const DiffArgs* dx, hipStream_t stream)
{
  switch (p)
  {
  case 1:
    return launch_cell_p<1, MODE>(d, a, c, ustride, ystride, rx, dx, stream);
  case 2:
    return launch_cell_p<2, MODE>(d, a, c, ustride, ystride, rx, dx, stream);
  case 3:
    return launch_cell_p<3, MODE>(d, a, c, ustride, ystride, rx, dx, stream);
  default:
    return launch_cell_p<4, MODE>(d, a, c, ustride, ystride, rx, dx, stream);
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
  const ReactArgs rx = react_args(h);
  const DiffArgs dx{h.diff.get()};
  return launch_cell<MODE>(h.p, d, a, c, h.ndofs, (int64_t)h.space.ncells * h.nd, h.has_react ? &rx : nullptr,
                           h.has_diff ? &dx : nullptr, stream);
}
} // namespace

void primal_level(eqlb_primal* h, SolverLevel& v) { solver_level(h, v); }
void primal_matrix_view(eqlb_primal* h, MatrixView& v) { solver_matrix_view(h, v); }
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

int eqlb_get_mass_table(int32_t p, double* out, int32_t capacity)
{
  using namespace eqlb;
  if (p < 1 || p > PS_PMAX || !out)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_get_mass_table: p = %d outside 1 ... 4, or null output", (int)p);
  const int n = nd_of(p) * nd_of(p);
  if (capacity < n)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_get_mass_table: capacity too small");
  const double* t = p == 1 ? eqlb_tables::Mass<1>::MS
                           : p == 2 ? eqlb_tables::Mass<2>::MS
                                    : p == 3 ? eqlb_tables::Mass<3>::MS : eqlb_tables::Mass<4>::MS;
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

int eqlb_primal_set_reaction(eqlb_primal_t* h, double c, const double* cell_c, int32_t memspace, void* stream_)
try
{
  return eqlb::solver_set_reaction("eqlb_primal_set_reaction", h, c, cell_c, memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_primal_set_diffusion(eqlb_primal_t* h, const double* cell_D, int32_t memspace, void* stream_)
try
{
  return eqlb::solver_set_diffusion("eqlb_primal_set_diffusion", h, cell_D, memspace, stream_);
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
