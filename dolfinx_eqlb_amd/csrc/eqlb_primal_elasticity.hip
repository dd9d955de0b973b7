// The P_p^2 linear-elasticity problem -div(2 eps(u) + pi_1 div(u) I) = f ON THE DEVICE: the counterpart of
// eqlb_primal_solve.hip for the displacement eqlb_primal_stress_dg takes - the primal solve of the reference's
// demo/elasticity_adaptive/demo_cook.py, which no DOLFINx can do on a mesh that was refined on the device.  The space is
// the scalar numbering of eqlb_mesh_lagrange_dofmap, blocked: u[2 dof + r].  The rule is stated in include/eqlb.h and,
// as numpy, in dolfinx_eqlb_amd/lsolver/primal.py (ElasticityOperator); operator, load, diagonal and residual
// reproduce the numpy statement bit for bit.
//
// The rule of a cell (no fused multiply-add anywhere; K = J^-1 as eqlb_primal_solve.hip forms it, K[X][d]):
//   Q[a][b][X][Y] = K[X][a] K[Y][b]
//   g_XY^s[i] = sum_j M_XY[i][j] u_s[j], ascending j, every product rounded on its own, with M_00 = S0 = Stiff<P>[0],
//               M_01 = Cross<P>, M_10 = Cross<P>^T, M_11 = S2 = Stiff<P>[2]
//   D_ab^s[i] = (Q[a][b][0][0] g_00^s[i] + Q[a][b][0][1] g_01^s[i]) + (Q[a][b][1][0] g_10^s[i] + Q[a][b][1][1] g_11^s[i])
//   y_loc[c][i][0] = |det J| (((D_00^0 + D_11^0) + (D_00^0 + D_10^1)) + pi_c (D_00^0 + D_01^1))
//   y_loc[c][i][1] = |det J| (((D_00^1 + D_11^1) + (D_01^0 + D_11^1)) + pi_c (D_10^0 + D_11^1))
//   diagonal (i, r): g_XY = M_XY[i][i], D_ab as above, |det J| (((D_00 + D_11) + D_rr) + pi_c D_rr)
//   load (i, r):     |det J| sum_n Load<P, D>[i][n] f_r[c][n], ascending n
//
//  k_elast_cell<P, MODE, D>  one thread per cell, ES_THREADS = 128 cells per workgroup: the 2 nd_p output values of a
//    cell are staged in LDS as k_primal_cell stages its nd_p, and at P = 4 the rows of 256 cells (62 KB) and the tables
//    would not fit a static block; 128 cells need 31 KB + 5.4 KB.  The tables (S0, S2, Cross: 3 nd_p^2 doubles; or
//    Load<P, D>) are read as a broadcast, the index rows of the workgroup move through LDS as one contiguous piece, and
//    so do the output rows y_loc [ncells][nd_p][2].
//  k_primal_gather<2, 1>, k_pcg_*<1>, pcg_solve: eqlb_primal_common.h, on one column of n = 2 ndofs rows with the
//    mask per row.
// This unit holds the cell kernel, its dispatch on p and d, the table getter and the C entries; the handle, the
// launches on it and the bodies of the C entries are those of eqlb_primal_handle.h at bs = 2 and one column.
#include "eqlb_device_common.h"
#include "eqlb_primal_handle.h" // the host side of a solver handle; eqlb_primal_common.h: the kernels it launches
#include "eqlb_tables_gen.h"

#include <algorithm>
#include <cmath>
#include <vector>

// the handle behind eqlb_elasticity_t; the per-cell coefficient of the base is cell_pi1
struct eqlb_elasticity : eqlb::SolverHandle<2, 1>
{
  double pi_1 = 1.0;
  eqlb::CellTerm shear{eqlb::SHEAR}; // the shear modulus (solver_set_cell_term): off (mu = 1) as created
};

namespace eqlb
{
namespace
{
constexpr int ES_THREADS = 128; // cells per workgroup of the cell kernel

struct ElastCellArgs
{
  int32_t ncells;
  const int32_t* cell_dofs; // [ncells][nd_p], the scalar numbering
  const double *cellJ, *cell_pi1;
  double pi_1;
  const double* u;      // operator: [2 ndofs] blocked; load: rhs_dg [2][ncells][nd_d]
  const uint8_t* fixed; // [2 ndofs]; operator, only_fixed: the free rows of u read as 0
  int32_t only_fixed;
  double* yloc; // [ncells][nd_p][2]
  const PcgState* st;
};

// The kernel with the reaction term (include/eqlb.h) is k_elast_cell_react, from the same source
// (eqlb_primal_elast_cell.inc): Mass<P> is staged behind the three tables and wm m^r[i] (diagonal: wm Mass[i][i]) is
// added to the value formed without the term.  A kernel of its own, so that a handle without the term launches the
// instantiations - symbols, arguments and code - it launched before the term existed.
//
// The kernels with a cell-wise shear modulus (eqlb_elasticity_set_shear) are k_elast_cell_shear and
// k_elast_cell_react_shear, again from the same source: y_loc = mu_T v with v the value formed without the term, then
// + wm m as above.  The coefficient is a kernel argument of its own (ShearArgs), as ReactArgs is.
#define EQLB_CELL_SHEAR 0
#define EQLB_CELL_REACT 0
#include "eqlb_primal_elast_cell.inc"
#undef EQLB_CELL_REACT
#define EQLB_CELL_REACT 1
#include "eqlb_primal_elast_cell.inc"
#undef EQLB_CELL_REACT
#undef EQLB_CELL_SHEAR
#define EQLB_CELL_SHEAR 1
#define EQLB_CELL_REACT 0
#include "eqlb_primal_elast_cell.inc"
#undef EQLB_CELL_REACT
#define EQLB_CELL_REACT 1
#include "eqlb_primal_elast_cell.inc"
#undef EQLB_CELL_REACT
#undef EQLB_CELL_SHEAR

// ---- host side ------------------------------------------------------------------------------------------------
template <int P, int MODE>
hipError_t launch_cell_d(int d, const ElastCellArgs& a, const ReactArgs* rx, const ShearArgs* sx, hipStream_t stream)
{
  const dim3 grid(grid_of(a.ncells, ES_THREADS)), block(ES_THREADS);
  if constexpr (MODE != CELL_LOAD)
  {
    // the variant with the terms the handle has; without one the launch as before the terms existed
    if (rx && sx)
      hipLaunchKernelGGL((k_elast_cell_react_shear<P, MODE, 0>), grid, block, 0, stream, a, *rx, *sx);
    else if (sx)
      hipLaunchKernelGGL((k_elast_cell_shear<P, MODE, 0>), grid, block, 0, stream, a, *sx);
    else if (rx)
      hipLaunchKernelGGL((k_elast_cell_react<P, MODE, 0>), grid, block, 0, stream, a, *rx);
    else
      hipLaunchKernelGGL((k_elast_cell<P, MODE, 0>), grid, block, 0, stream, a);
  }
  else
    switch (d)
    {
    case 0:
      hipLaunchKernelGGL((k_elast_cell<P, MODE, 0>), grid, block, 0, stream, a);
      break;
    case 1:
      hipLaunchKernelGGL((k_elast_cell<P, MODE, 1>), grid, block, 0, stream, a);
      break;
    case 2:
      hipLaunchKernelGGL((k_elast_cell<P, MODE, 2>), grid, block, 0, stream, a);
      break;
    default:
      hipLaunchKernelGGL((k_elast_cell<P, MODE, 3>), grid, block, 0, stream, a);
    }
  return hipGetLastError();
}

template <int MODE>
hipError_t launch_cell(int p, int d, const ElastCellArgs& a, const ReactArgs* rx, const ShearArgs* sx,
                       hipStream_t stream)
{
  switch (p)
  {
  case 1:
    return launch_cell_d<1, MODE>(d, a, rx, sx, stream);
  case 2:
    return launch_cell_d<2, MODE>(d, a, rx, sx, stream);
  case 3:
    return launch_cell_d<3, MODE>(d, a, rx, sx, stream);
  default:
    return launch_cell_d<4, MODE>(d, a, rx, sx, stream);
  }
}

// the hook of eqlb_primal_handle.h, the store pass on the one column of c: u [2 ndofs] (load: rhs_dg) into the y_loc of
// the handle
template <int MODE>
hipError_t launch_cell(const eqlb_elasticity& h, const ManyCols& c, int d, const double* u, bool only_fixed,
                       hipStream_t stream)
{
  ElastCellArgs a{};
  a.ncells = h.space.ncells;
  a.cell_dofs = h.cell_dofs;
  a.cellJ = h.mesh->m.cellJ;
  a.cell_pi1 = h.has_coeff ? h.coeff.get() : nullptr;
  a.pi_1 = h.pi_1;
  a.u = u;
  a.fixed = h.fixed;
  a.only_fixed = only_fixed ? 1 : 0;
  a.yloc = h.yloc;
  a.st = c.check ? c.st : nullptr;
  const ReactArgs rx = react_args(h.react);
  const ShearArgs sx = shear_args(h.shear);
  return launch_cell<MODE>(h.p, d, a, h.react.on ? &rx : nullptr, h.shear.on ? &sx : nullptr, stream);
}

// ---- the spring term (include/eqlb.h: eqlb_elasticity_set_springs) -------------------------------------------------
// the tests on a spring tensor (k00, k01, k11): what is refused, and what counts as positive definite.  The allowance
// 2^-49 lets a rank-one tensor formed in floating point as kn n_a n_b pass as semidefinite and not as definite
constexpr double SPRING_ALLOWANCE = 0x1p-49;
inline bool spring_semidefinite(const double* k)
{
  return !(k[1] * k[1] > (k[0] * k[2]) * (1.0 + SPRING_ALLOWANCE));
}
inline bool spring_definite(const double* k)
{
  return k[0] > 0.0 && k[1] * k[1] < (k[0] * k[2]) * (1.0 - SPRING_ALLOWANCE);
}

// the body of eqlb_elasticity_set_springs: the planner of a facet term (facet_term_plan) with alpha = 1, so that its
// weights are the lengths |E_f|; the tensors are looked at and weighted on the host (O(sqrt N) facets, one product per
// entry), and only then everything is put in the place of the old arrays: a refused call leaves the handle as it was.
int elasticity_set_springs(const char* who, eqlb_elasticity* h, int32_t nlist, const int32_t* facets, double k,
                           const double* facet_k, int32_t memspace, void* stream_)
{
  EQLB_TRY(check_handle(who, h));
  EQLB_TRY(check_memspace(who, memspace));
  EQLB_TRY(check_facet_list(who, nlist, facets));
  if (!facet_k && !(k >= 0.0 && std::isfinite(k)))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: k = %g is negative, NaN or infinite", who, k);
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool host = memspace == EQLB_MEM_HOST;
  if (nlist == 0)
    return solver_facet_term_off(h, memspace, stream);
  const size_t n = (size_t)nlist;
  std::vector<double> hk(6 * n); // Kw [n][3] | K [n][3]
  double* K = hk.data() + 3 * n;
  if (!facet_k)
    for (size_t i = 0; i < n; ++i)
    {
      K[3 * i] = K[3 * i + 2] = k;
      K[3 * i + 1] = 0.0;
    }
  else if (host)
    std::copy(facet_k, facet_k + 3 * n, K);
  else
  {
    HIP_TRY(hipMemcpyAsync(K, facet_k, 3 * n * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
  }
  FacetTermPlan plan;
  EQLB_TRY(facet_term_plan(
      who, h->mesh, h->p, h->ndofs, PS_THREADS / 2, nlist, facets, 1.0, nullptr, memspace, stream,
      [&](int32_t i) {
        const double* t = K + 3 * (size_t)i;
        if (!(std::isfinite(t[0]) && std::isfinite(t[1]) && std::isfinite(t[2])))
          return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: facet_k[%d] = (%g, %g, %g) is not finite", who, (int)i, t[0], t[1],
                      t[2]);
        if (t[0] < 0.0)
          return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: facet_k[%d]: k00 = %g is negative", who, (int)i, t[0]);
        if (t[2] < 0.0)
          return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: facet_k[%d]: k11 = %g is negative", who, (int)i, t[2]);
        if (!spring_semidefinite(t))
          return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: facet_k[%d] = (%g, %g, %g) is not positive semidefinite", who,
                      (int)i, t[0], t[1], t[2]);
        return (int)EQLB_OK;
      },
      plan));
  bool positive = false;
  for (size_t i = 0; i < n; ++i)
  {
    const bool listed = plan.flag[i] == 1;
    const double len = plan.w[i]; // (alpha = 1: the length)
    for (int c = 0; c < 3; ++c)
      hk[3 * i + c] = listed ? len * K[3 * i + c] : 0.0;
    positive = positive || (listed && len > 0.0 && spring_definite(K + 3 * i));
  }
  DevBuf<double> kw;
  if (kw.alloc_raw(6 * n) != hipSuccess)
    return fail(EQLB_ERR_NO_MEMORY, "%s: device allocation failed", who);
  HIP_TRY(hipMemcpyAsync(kw.get(), hk.data(), 6 * n * sizeof(double), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipStreamSynchronize(stream)); // (hk ends with this call)
  return solver_facet_term_commit(h, plan, nlist, positive, memspace, stream, &kw);
}
} // namespace

void elasticity_level(eqlb_elasticity* h, SolverLevel& v) { solver_level(h, v); }
void elasticity_matrix_view(eqlb_elasticity* h, MatrixView& v)
{
  solver_matrix_view(h, v);
  v.pi_1 = h->pi_1;
  v.has_shear = h->shear.on;
  v.sx = shear_args(h->shear);
}
} // namespace eqlb

extern "C" {

int eqlb_get_cross_table(int32_t p, double* out, int32_t capacity)
{
  using namespace eqlb;
  if (p < 1 || p > PS_PMAX || !out)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_get_cross_table: p = %d outside 1 ... 4, or null output", (int)p);
  const int n = nd_of(p) * nd_of(p);
  if (capacity < n)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_get_cross_table: capacity too small");
  const double* t = p == 1 ? eqlb_tables::Cross<1>::CR
                           : p == 2 ? eqlb_tables::Cross<2>::CR
                                    : p == 3 ? eqlb_tables::Cross<3>::CR : eqlb_tables::Cross<4>::CR;
  for (int i = 0; i < n; ++i)
    out[i] = t[i];
  return n;
}

int eqlb_elasticity_create(eqlb_mesh_t* mesh, int32_t p, double pi_1, const double* cell_pi1, int32_t memspace,
                           void* stream_, eqlb_elasticity_t** handle)
try
{
  auto h = std::make_unique<eqlb_elasticity>();
  h->pi_1 = pi_1;
  return eqlb::solver_create("eqlb_elasticity_create", std::move(h), mesh, p, cell_pi1, memspace, stream_, handle);
}
EQLB_CATCH_ALL

void eqlb_elasticity_destroy(eqlb_elasticity_t* handle) { delete handle; }

int eqlb_elasticity_ndofs(const eqlb_elasticity_t* handle, int64_t* ndofs)
{
  return eqlb::solver_ndofs("eqlb_elasticity_ndofs", handle, ndofs);
}

int eqlb_elasticity_set_dirichlet(eqlb_elasticity_t* h, int32_t nlist0, const int32_t* facets0, int32_t nlist1,
                                  const int32_t* facets1, int32_t memspace, void* stream_)
try
{
  const int32_t nlists[2] = {nlist0, nlist1};
  const int32_t* const lists[2] = {facets0, facets1};
  return eqlb::solver_set_dirichlet("eqlb_elasticity_set_dirichlet", h, nlists, lists, memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_elasticity_set_reaction(eqlb_elasticity_t* h, double c, const double* cell_c, int32_t memspace, void* stream_)
try
{
  return eqlb::solver_set_cell_term("eqlb_elasticity_set_reaction", h, eqlb::REACTION, &eqlb_elasticity::react, c,
                                    cell_c, memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_elasticity_set_shear(eqlb_elasticity_t* h, double mu, const double* cell_mu, int32_t memspace, void* stream_)
try
{
  return eqlb::solver_set_cell_term("eqlb_elasticity_set_shear", h, eqlb::SHEAR, &eqlb_elasticity::shear, mu, cell_mu,
                                    memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_elasticity_set_springs(eqlb_elasticity_t* h, int32_t nlist, const int32_t* facets, double k,
                                const double* facet_k, int32_t memspace, void* stream_)
try
{
  return eqlb::elasticity_set_springs("eqlb_elasticity_set_springs", h, nlist, facets, k, facet_k, memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_elasticity_spring_weights(eqlb_elasticity_t* h, int32_t* nlist, double* kw, int32_t capacity,
                                   int32_t memspace, void* stream_)
try
{
  return eqlb::solver_facet_weights("eqlb_elasticity_spring_weights", h, nlist, kw, capacity, memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_elasticity_spring_flux(eqlb_elasticity_t* h, const double* u, int32_t nq, const double* s,
                                const double* u_ext, double* out, int32_t memspace, void* stream_)
try
{
  return eqlb::solver_facet_flux("eqlb_elasticity_spring_flux", "spring", "eqlb_elasticity_set_springs", h, u, nq, s,
                                 u_ext, out, memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_elasticity_load(eqlb_elasticity_t* h, int32_t degree_dg, const double* rhs_dg, const double* b_extra,
                         double* b, int32_t memspace, void* stream_)
try
{
  return eqlb::solver_load("eqlb_elasticity_load", h, degree_dg, rhs_dg, b_extra, b, memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_elasticity_apply(eqlb_elasticity_t* h, const double* u, double* y, int32_t masked, int32_t memspace,
                          void* stream_)
try
{
  return eqlb::solver_apply("eqlb_elasticity_apply", h, 1, u, y, masked, memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_elasticity_diagonal(eqlb_elasticity_t* h, double* out, int32_t memspace, void* stream_)
try
{
  return eqlb::solver_diagonal("eqlb_elasticity_diagonal", h, out, memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_elasticity_residual(eqlb_elasticity_t* h, const double* b, const double* u, double* r, double* norms,
                             int32_t memspace, void* stream_)
try
{
  return eqlb::solver_residual("eqlb_elasticity_residual", h, b, u, r, norms, memspace, stream_);
}
EQLB_CATCH_ALL

int eqlb_elasticity_solve(eqlb_elasticity_t* h, const double* b, double* u, double rtol, double atol, int32_t maxit,
                          double* info, int32_t memspace, void* stream_)
try
{
  return eqlb::solver_solve("eqlb_elasticity_solve", h, 1, b, u, rtol, atol, maxit, info, memspace, stream_);
}
EQLB_CATCH_ALL

} // extern "C"

