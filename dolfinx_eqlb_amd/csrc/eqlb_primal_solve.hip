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

#include <algorithm>
#include <functional>
#include <cmath>
#include <unordered_set>
#include <vector>

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
  const ReactArgs rx = react_args(h.react);
  const DiffArgs dx = diff_args(h.diff);
  return launch_cell<MODE>(h.p, d, a, c, h.ndofs, (int64_t)h.space.ncells * h.nd, h.react.on ? &rx : nullptr,
                           h.diff.on ? &dx : nullptr, stream);
}
// ---- the Robin term (include/eqlb.h: eqlb_primal_set_robin) --------------------------------------------------------
// One thread per listed facet: its rows in the local order (lower node id, higher node id, nnodes + f (p-1) + j), its
// weight w = alpha |E| with |E| = sqrt(dx dx + dy dy) from facet_nodes, every operation rounded on its own, and what the
// host needs to refuse or skip it: flag 1 a boundary facet, 2 a facet between two cells, 0 an id or a node outside the
// mesh (nothing of it is read).  A facet that is not flagged 1 gets the weight 0 and the rows -1.
__global__ void __launch_bounds__(PS_THREADS)
k_robin_prepare(int32_t nlist, const int32_t* __restrict__ facets, double alpha, const double* __restrict__ facet_alpha,
                int32_t nnodes, int32_t nfacets, int32_t ne, const double* __restrict__ x,
                const int32_t* __restrict__ facet_nodes, const int32_t* __restrict__ fco, int32_t* __restrict__ flist,
                int32_t* __restrict__ dofs, int32_t* __restrict__ flag, double* __restrict__ w, double* __restrict__ al)
{
#pragma clang fp contract(off)
  const int32_t i = blockIdx.x * PS_THREADS + threadIdx.x;
  if (i >= nlist)
    return;
  const int32_t f = facets[i];
  const double a = facet_alpha ? facet_alpha[i] : alpha;
  int32_t* dd = dofs + (int64_t)i * FACET_ROW;
  int32_t fl = 0, n0 = -1, n1 = -1;
  if (f >= 0 && f < nfacets)
  {
    n0 = facet_nodes[2 * (int64_t)f];
    n1 = facet_nodes[2 * (int64_t)f + 1];
    if (n0 >= 0 && n0 < nnodes && n1 >= 0 && n1 < nnodes)
      fl = (fco[f + 1] - fco[f] == 1) ? 1 : 2;
  }
  flist[i] = f;
  flag[i] = fl;
  al[i] = a;
  if (fl != 1)
  {
    w[i] = 0.0;
    for (int j = 0; j < FACET_ROW; ++j)
      dd[j] = -1;
    return;
  }
  const double dx = x[3 * (int64_t)n1] - x[3 * (int64_t)n0], dy = x[3 * (int64_t)n1 + 1] - x[3 * (int64_t)n0 + 1];
  w[i] = a * sqrt(dx * dx + dy * dy);
  dd[0] = n0 < n1 ? n0 : n1;
  dd[1] = n0 < n1 ? n1 : n0;
  for (int j = 0; j < FACET_ROW - 2; ++j)
    dd[2 + j] = j < ne ? nnodes + f * ne + j : -1;
}

const double* facet_mass_of(int p)
{
  return p == 1 ? eqlb_tables::FacetMass<1>::FM
                : p == 2 ? eqlb_tables::FacetMass<2>::FM
                         : p == 3 ? eqlb_tables::FacetMass<3>::FM : eqlb_tables::FacetMass<4>::FM;
}

} // namespace

// The planner of a facet term (eqlb_primal_handle.h: FacetTermPlan), shared by eqlb_primal_set_robin and
// eqlb_elasticity_set_springs.  The list (nlist >= 1) is prepared on the device into fresh arrays, looked at on the
// host, where the table of the sum pass is built (the listed facets are O(sqrt N)); nothing of a handle is touched, so
// that a refused call leaves it as it was.  The call waits for the stream in both memory spaces.
int facet_term_plan(const char* who, eqlb_mesh* mesh, int p, int64_t ndofs, int chunk_dofs, int32_t nlist,
                    const int32_t* facets, double alpha, const double* facet_alpha, int32_t memspace, hipStream_t stream,
                    const std::function<int(int32_t)>& refuse, FacetTermPlan& out)
{
  const bool host = memspace == EQLB_MEM_HOST;
  const DeviceMesh& m = mesh->m;
  const size_t n = (size_t)nlist;
  const int n1 = p + 1;
  DevBuf<double>& val = out.val;
  DevBuf<int32_t> head; // facets | dofs | flag
  if (val.alloc_raw(2 * n + (size_t)n1 * n1) != hipSuccess || head.alloc_raw(n * (2 + FACET_ROW)) != hipSuccess)
    return fail(EQLB_ERR_NO_MEMORY, "%s: device allocation failed", who);
  std::vector<int32_t> hh(n * (2 + FACET_ROW));
  std::vector<double>& hw = out.w;
  hw.assign(n, 0.0);
  {
    HostCall s;
    const auto d_f = s.in(host ? facets : nullptr, n);
    const auto d_a = s.in(host ? facet_alpha : nullptr, n);
    if (host)
      HIP_TRY(s.upload(stream));
    int32_t* flist = head.get();
    hipLaunchKernelGGL(k_robin_prepare, dim3(grid_of(nlist, PS_THREADS)), dim3(PS_THREADS), 0, stream, nlist,
                       host ? d_f.get() : facets, alpha, host ? d_a.get() : facet_alpha, m.nnodes, m.nfacets, p - 1,
                       m.x, m.facet_nodes, m.facet_cells_off, flist, flist + n, flist + n * (1 + FACET_ROW), val.get(),
                       val.get() + n);
    s.note(hipGetLastError());
    s.note(hipMemcpyAsync(val.get() + 2 * n, facet_mass_of(p), (size_t)n1 * n1 * sizeof(double),
                          hipMemcpyHostToDevice, stream));
    s.note(hipMemcpyAsync(hh.data(), head.get(), hh.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    s.note(hipMemcpyAsync(hw.data(), val.get(), n * sizeof(double), hipMemcpyDeviceToHost, stream));
    s.note(hipStreamSynchronize(stream));
    HIP_TRY(s.finish(stream));
  }
  const int32_t* hd = hh.data() + n;
  const int32_t* hflag = hh.data() + n * (1 + FACET_ROW);
  if (host)
  {
    std::unordered_set<int32_t> seen;
    for (int32_t i = 0; i < nlist; ++i)
    {
      if (hflag[i] != 1)
        return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: facets[%d] = %d is no boundary facet of the mesh", who, (int)i,
                    (int)facets[i]);
      if (!seen.insert(facets[i]).second)
        return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: facets[%d] = %d is listed twice", who, (int)i, (int)facets[i]);
      EQLB_TRY(refuse(i));
    }
  }
  // the table of the sum pass (eqlb_facet_plan.h), in one array behind the facets and dofs as the device left them in hh
  const FacetTable t = facet_plan(n, hflag, hh.data(), hd, n1, ndofs, chunk_dofs);
  const FacetLayout& at = t.at;
  std::vector<int32_t> tab(at.total);
  std::copy(hh.begin(), hh.begin() + (std::ptrdiff_t)at.chunk, tab.begin());
  std::copy(t.chunk.begin(), t.chunk.end(), tab.begin() + (std::ptrdiff_t)at.chunk);
  std::copy(t.rows.begin(), t.rows.end(), tab.begin() + (std::ptrdiff_t)at.rows);
  std::copy(t.off.begin(), t.off.end(), tab.begin() + (std::ptrdiff_t)at.off);
  std::copy(t.ent.begin(), t.ent.end(), tab.begin() + (std::ptrdiff_t)at.ent);
  DevBuf<int32_t>& dtab = out.tab;
  if (dtab.alloc_raw(at.total) != hipSuccess)
    return fail(EQLB_ERR_NO_MEMORY, "%s: device allocation failed", who);
  HIP_TRY(hipMemcpyAsync(dtab.get(), tab.data(), at.total * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipStreamSynchronize(stream)); // (tab ends with this call; nothing on the stream reads the old table any more)
  out.at = at;
  out.flag.assign(hflag, hflag + n);
  return EQLB_OK;
}

namespace
{
// the body of eqlb_primal_set_robin: the plan above, and only then the new arrays in the place of the old ones
int primal_set_robin(const char* who, eqlb_primal* h, int32_t nlist, const int32_t* facets, double alpha,
                     const double* facet_alpha, int32_t memspace, void* stream_)
{
  EQLB_TRY(check_handle(who, h));
  EQLB_TRY(check_memspace(who, memspace));
  EQLB_TRY(check_facet_list(who, nlist, facets));
  if (!facet_alpha)
    EQLB_TRY(check_scalar(who, "alpha", *FACET_ALPHA.rule, alpha));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (nlist == 0)
    return solver_facet_term_off(h, memspace, stream);
  FacetTermPlan plan;
  EQLB_TRY(facet_term_plan(
      who, h->mesh, h->p, h->ndofs, PS_THREADS, nlist, facets, alpha, facet_alpha, memspace, stream,
      [&](int32_t i) {
        return facet_alpha && !FACET_ALPHA.rule->ok(facet_alpha[i]) ? fail_cell(who, FACET_ALPHA, facet_alpha, i) : EQLB_OK;
      },
      plan));
  bool positive = false;
  for (int32_t i = 0; i < nlist; ++i)
    positive = positive || (plan.flag[(size_t)i] == 1 && plan.w[(size_t)i] > 0.0);
  return solver_facet_term_commit(h, plan, nlist, positive, memspace, stream);
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
  return eqlb::solver_set_cell_term("eqlb_primal_set_reaction", h, eqlb::REACTION, &eqlb_primal::react, c, cell_c,
                                    memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_primal_set_diffusion(eqlb_primal_t* h, const double* cell_D, int32_t memspace, void* stream_)
try
{
  return eqlb::solver_set_cell_term("eqlb_primal_set_diffusion", h, eqlb::DIFFUSION, &eqlb_primal::diff, 0.0, cell_D,
                                    memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_get_facet_mass_table(int32_t p, double* out, int32_t capacity)
{
  using namespace eqlb;
  if (p < 1 || p > PS_PMAX || !out)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_get_facet_mass_table: p = %d outside 1 ... 4, or null output", (int)p);
  const int n = (p + 1) * (p + 1);
  if (capacity < n)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_get_facet_mass_table: capacity too small");
  const double* t = facet_mass_of(p);
  for (int i = 0; i < n; ++i)
    out[i] = t[i];
  return n;
}

int eqlb_primal_set_robin(eqlb_primal_t* h, int32_t nlist, const int32_t* facets, double alpha,
                          const double* facet_alpha, int32_t memspace, void* stream_)
try
{
  return eqlb::primal_set_robin("eqlb_primal_set_robin", h, nlist, facets, alpha, facet_alpha, memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_primal_robin_weights(eqlb_primal_t* h, int32_t* nlist, double* w, int32_t capacity, int32_t memspace,
                              void* stream_)
try
{
  return eqlb::solver_facet_weights("eqlb_primal_robin_weights", h, nlist, w, capacity, memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_primal_robin_flux(eqlb_primal_t* h, const double* u, int32_t nq, const double* s, const double* u_ext,
                           double* out, int32_t memspace, void* stream_)
try
{
  return eqlb::solver_facet_flux("eqlb_primal_robin_flux", "Robin", "eqlb_primal_set_robin", h, u, nq, s, u_ext, out,
                                 memspace, stream_);
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
