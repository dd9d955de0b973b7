// The host side of a P_p solver handle, ONCE for the Poisson unit (eqlb_primal_solve.hip: eqlb_primal, bs = 1, up to
// MANY_R columns) and the elasticity unit (eqlb_primal_elasticity.hip: eqlb_elasticity, bs = 2, one column): the
// handle base, the launches on its work space, the view the hierarchy unit gets and the bodies of the C entries.  A unit
// adds its cell kernel and, for its handle type H, the one hook the code here finds by overload:
//   template <int MODE> hipError_t launch_cell(const H&, const ManyCols&, int d, const double* u, bool only_fixed,
//                                              hipStream_t)
// the store pass on the columns of c (u [R][bs ndofs]; load: rhs_dg of degree d) into the y_loc of work_of(h, c.R).
// bs and the column limit are constants of H, so a unit instantiates the kernels of its own bs and column count only.
// Everything lies in an unnamed namespace, as in eqlb_primal_common.h.
//
// THE STATUS WORD of a handle, int32 [4] in device memory:
//   [0]        listed facet ids outside the mesh, skipped (device memory space only; info[7] of a solve)
//   [1 .. bs]  listed valid ids of component 0 .. bs - 1: a solve refuses a component without one as singular
//   [1 + bs]   slots of the sum pass that matched no local index (a broken table), counted at create
// set_dirichlet clears the 1 + bs words of the mask and leaves the last one; k_primal_slots counts in the third word
// behind its status pointer, so it gets status + (bs - 1).
#pragma once

#include "eqlb_mesh_handle.h" // (eqlb_host_util.h)
#include "eqlb_primal_common.h"

#include <climits>
#include <functional>
#include <memory>
#include <vector>

namespace eqlb
{
// The CSR pattern of a handle's operator (include/eqlb.h: eqlb_primal_matrix_pattern), built once by
// eqlb_primal_matrix.hip and kept until eqlb_*_matrix_release or the end of the handle.  It is the SCALAR pattern - the
// sorted distinct pairs (d, d') of DOFs with a common cell; the bs * bs blocked entries of a pair follow from it by
// index arithmetic (row bs d + r: first bs bs sptr[d] + r bs len(d), then bs k + s), so a [P_p]^2 handle stores a
// quarter of its index arrays.
struct MatrixPattern
{
  bool built = false;
  int64_t snnz = 0;           // pairs; the matrix has bs * bs * snnz entries
  DevBuf<int64_t> sptr;       // [ndofs + 1] first pair of a DOF's row
  DevBuf<int32_t> srow, scol; // [snnz] the DOFs of a pair
  size_t peak_bytes = 0;      // device memory at the peak of the build, the kept arrays included
};

namespace
{
// the reaction term of a cell kernel (include/eqlb.h): c_T = cell_c[cell] where given, else the scalar c.  A kernel
// argument of its own, which the kernels without the term do not take.
struct ReactArgs
{
  const double* cell_c = nullptr; // [ncells] or nullptr
  double c = 0.0;
};

// the shear modulus of the elasticity cell kernel (include/eqlb.h): mu_T = cell_mu[cell] where given, else the scalar mu.
// A kernel argument of its own, which the kernels without the term do not take.
struct ShearArgs
{
  const double* cell_mu = nullptr; // [ncells] or nullptr
  double mu = 1.0;
};

// the diffusion tensor of the Poisson cell kernel (include/eqlb.h): D_T = (d00, d01, d11) = cell_D[cell].  A kernel
// argument of its own, which the kernels without the term do not take.
struct DiffArgs
{
  const double* cell_D = nullptr; // [ncells][3]
};
} // namespace

// A solver handle as eqlb_primal_matrix.hip sees it: a view that owns nothing, all pointers DEVICE.  coeff: kappa
// (bs = 1) or pi_1 (bs = 2) per cell, or nullptr (1, or the scalar pi_1).  The space and the terms come as the kernel
// arguments the handle hands out (the same plain structs in every unit that sees the view)
struct MatrixView
{
  int bs = 1, p = 0;
  SpaceArgs s{};
  const int32_t* cell_dofs = nullptr;
  const double *cellJ = nullptr, *coeff = nullptr;
  double pi_1 = 1.0;
  bool has_react = false, has_shear = false, has_diff = false;
  ReactArgs rx;
  ShearArgs sx;
  DiffArgs dx;
  const uint8_t* fixed = nullptr;
  MatrixPattern* pattern = nullptr;
  // the facet term, the table of a sum pass on the diagonal: facet_m DOFs lie in a listed facet
  bool has_facet = false;
  int32_t facet_m = 0;
  FacetTermArgs facet{};
};

// What the planner of a facet term leaves for the setter that called it (eqlb_primal_solve.hip: facet_term_plan): the
// device arrays a handle takes over, where the table's pieces lie (FacetLayout), and on the host the weight and the
// flag of every listed facet (1: a boundary facet; anything else was skipped).  `refuse` is asked per facet, in the
// order of the list and behind the tests on the facet itself, in host memory space: the caller's coefficient test.
// chunk_dofs: the DOFs of a chunk of PS_THREADS rows of the sum pass, PS_THREADS / bs.
struct FacetTermPlan
{
  DevBuf<int32_t> tab; // facets [n] | dofs [n][FACET_ROW] | chunk | rows [m] | off [m + 1] | ent
  DevBuf<double> val;  // w [n] = alpha_f |E_f| | alpha [n] | FacetMass<p> [(p + 1)^2]
  FacetLayout at;
  std::vector<double> w;
  std::vector<int32_t> flag;
};
int facet_term_plan(const char* who, eqlb_mesh* mesh, int p, int64_t ndofs, int chunk_dofs, int32_t nlist,
                    const int32_t* facets, double alpha, const double* facet_alpha, int32_t memspace, hipStream_t stream,
                    const std::function<int(int32_t)>& refuse, FacetTermPlan& out);
void primal_matrix_view(eqlb_primal* h, MatrixView& v);         // eqlb_primal_solve.hip
void elasticity_matrix_view(eqlb_elasticity* h, MatrixView& v); // eqlb_primal_elasticity.hip

namespace
{
// A per-cell term of a handle as its setter needs it (solver_set_cell_term): the array with its name and rule
// (eqlb_cell_coeff.h; its width follows from the rule), the name of the scalar in messages (nullptr: the term has
// none) and the scalar's neutral value, which without an array switches the term off
struct CellTermSpec
{
  CellCoeff array;
  const char* scalar;
  double neutral;
};
constexpr CellTermSpec REACTION{CELL_C, "c", 0.0}, SHEAR{CELL_MU, "mu", 1.0}, DIFFUSION{CELL_D, nullptr, 0.0};

// ... and as the handle holds it: off as created.  The array is allocated by the first call that brings one and kept;
// `cell` says whether the kernels read it or the scalar.  The kernel arguments are handed out below
struct CellTerm
{
  bool on = false, cell = false;
  double scalar;
  DevBuf<double> buf;
  explicit CellTerm(const CellTermSpec& d) : scalar(d.neutral) {}
  const double* array() const { return cell ? buf.get() : nullptr; }
};
inline ReactArgs react_args(const CellTerm& t) { return ReactArgs{t.array(), t.scalar}; }
inline ShearArgs shear_args(const CellTerm& t) { return ShearArgs{t.array(), t.scalar}; }
inline DiffArgs diff_args(const CellTerm& t) { return DiffArgs{t.array()}; }

// A facet term as the handle holds it - the Robin term of the Poisson unit (eqlb_primal_set_robin) or the spring term
// of the elasticity unit (eqlb_elasticity_set_springs): off as created.  The arrays are allocated by a setter that
// brings a list and replaced as a whole by the next one (solver_facet_term_commit).  A spring term has alpha = 1, so
// that the w of val are the lengths |E_f|, and its tensors in kw
struct FacetTerm
{
  bool on = false, positive = false; // positive: some weight > 0 - the operator is definite without a fixed DOF
  int32_t n = 0;                     // listed facets
  DevBuf<int32_t> tab;               // the pieces of FacetLayout ...
  FacetLayout at;                    // ... and where they lie
  DevBuf<double> val;                // w [n] | alpha [n] | FacetMass<p> [(p + 1)^2]
  DevBuf<double> kw;                 // bs = 2: Kw [n][3] = |E_f| (k00, k01, k11) | K [n][3]
};

// what eqlb_primal_t and eqlb_elasticity_t share; everything but the grown work space is carved out of one allocation at
// create
template <int BS, int MAXC>
struct SolverHandle
{
  static_assert((BS == 1 && MAXC == MANY_R) || (BS == 2 && MAXC == 1), "columns for scalar spaces only");
  static constexpr int bs = BS;         // components per DOF: the vectors have bs * ndofs rows
  static constexpr int max_cols = MAXC; // columns of a launch at the most
  eqlb_mesh* mesh = nullptr;
  int p = 0, nd = 0;
  int64_t ndofs = 0; // scalar count
  bool has_coeff = false;
  SpaceArgs space{};
  DevCarve mem;
  DevPiece<int32_t> cell_dofs, slots, status;
  DevPiece<double> coeff, yloc, diag, r, z, d, q, part; // coeff [ncells]: kappa, or pi_1 per cell
  DevPiece<uint8_t> fixed;
  DevPiece<PcgState> st;
  // the work space for 2 ... max_cols columns (wide.R of them): grown by the first call that needs it, then reused
  DevBuf<char> wide_mem;
  PcgWork wide{};
  // the reaction term and, for the Poisson unit, the diffusion tensor (solver_set_cell_term)
  CellTerm react{REACTION}, diff{DIFFUSION};
  FacetTerm facet;
  // the CSR pattern of the operator (eqlb_primal_matrix.hip): empty until eqlb_*_matrix_pattern
  MatrixPattern pattern;
};

constexpr int STATUS_WORDS = 4;

// the hook of a unit (above); this declaration only makes the name a template for the calls below
template <int MODE, class H>
hipError_t launch_cell(const H& h, const ManyCols& c, int d, const double* u, bool only_fixed, hipStream_t stream);

const ManyCols ONE_COLUMN{1, 1u, 0, nullptr}; // a launch on one vector that knows no state

// the work space the launches on R columns use: the carve of the handle for one, the grown one (primal_work) for more
template <class H>
PcgWork work_of(const H& h, int R)
{
  PcgWork w = R == 1 ? PcgWork{H::bs * h.ndofs, 1, h.diag, h.fixed, h.yloc, h.r, h.z, h.d, h.q, h.part, h.st} : h.wide;
  w.R = R;
  return w;
}

// the work space for R columns, grown if need be; a handle type of one column refuses more
template <class H>
int primal_work(H* h, int R, PcgWork& w)
{
  if constexpr (H::max_cols == 1)
  {
    if (R != 1)
      return fail(EQLB_ERR_UNSUPPORTED,
                  "elasticity_level: several right-hand sides are provided for Poisson handles (bs = 1) only");
  }
  else if (R > 1 && R > h->wide.R)
  {
    const size_t n = (size_t)H::bs * h->ndofs, ny = (size_t)H::bs * h->space.ncells * h->nd;
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
    h->wide = PcgWork{(int64_t)n, R,       h->diag, h->fixed, dp(o_y), dp(o_r),
                      dp(o_z),    dp(o_d), dp(o_q), dp(o_p),  reinterpret_cast<PcgState*>(base + o_s)};
  }
  w = work_of(*h, R);
  return EQLB_OK;
}

// the weights of the handle's facet term as the kernels of its bs read them, w [n] or Kw [n][3], and the coefficients
// behind them, alpha [n] or K [n][3]
template <class H>
const double* facet_weights(const H& h)
{
  return H::bs == 1 ? h.facet.val.get() : h.facet.kw.get();
}
template <class H>
const double* facet_coeffs(const H& h)
{
  return facet_weights(h) + (H::bs == 1 ? 1 : 3) * (size_t)h.facet.n;
}

// the table of the handle's facet term for a sum pass: u the vector of the store pass (column 0), nullptr: the diagonal
template <class H>
FacetTermArgs facet_args(const H& h, const double* u, bool only_fixed)
{
  FacetTermArgs x{};
  const int32_t* tab = h.facet.tab.get();
  const FacetLayout& at = h.facet.at;
  x.dofs = tab + at.dofs;
  x.chunk = tab + at.chunk;
  x.rows = tab + at.rows;
  x.off = tab + at.off;
  x.ent = tab + at.ent;
  x.w = facet_weights(h);
  x.fm = h.facet.val.get() + 2 * (size_t)h.facet.n;
  x.u = u;
  x.fixed = h.fixed;
  x.only_fixed = only_fixed ? 1 : 0;
  x.n1 = h.p + 1;
  return x;
}

template <class H>
GatherArgs gather_args(const H& h, const ManyCols& c, bool masked)
{
  const PcgWork w = work_of(h, c.R);
  GatherArgs g{};
  g.s = h.space;
  g.yloc = w.yloc;
  g.fixed = masked ? h.fixed.get() : nullptr;
  g.part = w.part;
  g.cols = c;
  g.ystride = (int64_t)H::bs * h.space.ncells * h.nd;
  return g;
}

template <class H>
hipError_t launch_gather(const H& h, const GatherArgs& g, hipStream_t stream)
{
  const dim3 grid(stream_blocks(H::bs * h.ndofs)), block(PS_THREADS);
  if constexpr (H::max_cols == 1)
    hipLaunchKernelGGL((k_primal_gather<H::bs, 1>), grid, block, 0, stream, g);
  else if (g.cols.R == 1)
    hipLaunchKernelGGL((k_primal_gather<H::bs, 1>), grid, block, 0, stream, g);
  else
    hipLaunchKernelGGL((k_primal_gather<H::bs, MANY_R>), grid, block, 0, stream, g);
  return hipGetLastError();
}

// the sum pass behind a store pass of the OPERATOR (u: what that pass read, nullptr: the diagonal): with a facet term
// on the handle the variant that adds the facet values, else the launch above.  The sum pass of the load and of the
// restriction of a hierarchy (enqueue_owner_sum) never carries the term
template <class H>
hipError_t launch_gather_op(const H& h, const GatherArgs& g, const double* u, bool only_fixed, hipStream_t stream)
{
  if (!h.facet.on)
    return launch_gather(h, g, stream);
  const dim3 grid(stream_blocks(H::bs * h.ndofs)), block(PS_THREADS);
  const FacetTermArgs x = facet_args(h, u, only_fixed);
  if constexpr (H::max_cols == 1)
    hipLaunchKernelGGL((k_primal_gather_facet<H::bs, 1>), grid, block, 0, stream, g, x);
  else if (g.cols.R == 1)
    hipLaunchKernelGGL((k_primal_gather_facet<H::bs, 1>), grid, block, 0, stream, g, x);
  else
    hipLaunchKernelGGL((k_primal_gather_facet<H::bs, MANY_R>), grid, block, 0, stream, g, x);
  return hipGetLastError();
}

// y = owner sum of y_loc (masked or raw) on the columns of c; y DEVICE [R][bs ndofs]
template <class H>
hipError_t enqueue_owner_sum(const H& h, const ManyCols& c, double* y, bool masked, hipStream_t stream)
{
  GatherArgs g = gather_args(h, c, masked);
  g.y = y;
  return launch_gather(h, g, stream);
}

template <class H>
hipError_t enqueue_diagonal(const H& h, double* out, hipStream_t stream)
{
  const hipError_t e = launch_cell<CELL_DIAGONAL>(h, ONE_COLUMN, 0, nullptr, false, stream);
  if (e != hipSuccess)
    return e;
  GatherArgs g = gather_args(h, ONE_COLUMN, false);
  g.y = out;
  return launch_gather_op(h, g, nullptr, false, stream);
}

// r = b - A u (0 on the fixed rows), u^ instead of u with only_fixed; the block partials of r.r are left in part
template <class H>
hipError_t enqueue_residual(const H& h, const ManyCols& c, const double* b, const double* u, double* r, bool only_fixed,
                            hipStream_t stream)
{
  const hipError_t e = launch_cell<CELL_OPERATOR>(h, c, 0, u, only_fixed, stream);
  if (e != hipSuccess)
    return e;
  GatherArgs g = gather_args(h, c, true);
  g.b = b;
  g.r = r;
  g.dot = DOT_R_R;
  return launch_gather_op(h, g, u, only_fixed, stream);
}

// q = A d on the free rows (the direction d of the work space), the block partials of d.q in part
template <class H>
hipError_t enqueue_product(const H& h, const ManyCols& c, hipStream_t stream)
{
  const PcgWork w = work_of(h, c.R);
  const hipError_t e = launch_cell<CELL_OPERATOR>(h, c, 0, w.d, false, stream);
  if (e != hipSuccess)
    return e;
  GatherArgs g = gather_args(h, c, true);
  g.y = w.q;
  g.w = w.d;
  g.dot = DOT_W_Y;
  return launch_gather_op(h, g, w.d, false, stream);
}

// the handle as the hierarchy unit sees it (eqlb_internal.h: SolverLevel)
template <class H>
void solver_level(H* h, SolverLevel& v)
{
  v = SolverLevel{};
  v.handle = h;
  v.mesh = h->mesh;
  v.p = h->p;
  v.bs = H::bs;
  v.ndofs = h->ndofs;
  v.cell_dofs = h->cell_dofs;
  v.diag = h->diag;
  v.fixed = h->fixed;
  v.status = h->status;
  v.work = [](void* hh, int R, PcgWork& w) { return primal_work(static_cast<H*>(hh), R, w); };
  v.owner_sum = [](void* hh, const ManyCols& c, double* y, bool masked, hipStream_t stream) {
    return enqueue_owner_sum(*static_cast<H*>(hh), c, y, masked, stream);
  };
  v.residual = [](void* hh, const ManyCols& c, const double* b, const double* u, double* r, bool only_fixed,
                  hipStream_t stream) {
    return enqueue_residual(*static_cast<H*>(hh), c, b, u, r, only_fixed, stream);
  };
  v.product = [](void* hh, const ManyCols& c, hipStream_t stream) {
    return enqueue_product(*static_cast<H*>(hh), c, stream);
  };
  v.definite = [](void* hh) { return static_cast<H*>(hh)->facet.on && static_cast<H*>(hh)->facet.positive; };
}

// the handle as the matrix unit sees it; a unit with further coefficients (pi_1, the shear modulus) adds them
template <class H>
void solver_matrix_view(H* h, MatrixView& v)
{
  v = MatrixView{};
  v.bs = H::bs;
  v.p = h->p;
  v.s = h->space;
  v.cell_dofs = h->cell_dofs;
  v.cellJ = h->mesh->m.cellJ;
  v.coeff = h->has_coeff ? h->coeff.get() : nullptr;
  v.has_react = h->react.on;
  v.rx = react_args(h->react);
  v.has_diff = h->diff.on;
  v.dx = diff_args(h->diff);
  v.fixed = h->fixed;
  v.pattern = &h->pattern;
  if (h->facet.on)
  {
    v.has_facet = true;
    v.facet_m = (int32_t)h->facet.at.m();
    v.facet = facet_args(*h, nullptr, false);
  }
}

// ---- the C entries behind their names (`who`) -------------------------------------------------------------------------
inline int check_handle(const char* who, const void* h)
{
  if (!h)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null handle", who);
  return EQLB_OK;
}

// what a setter of a facet term checks about its list
inline int check_facet_list(const char* who, int32_t nlist, const int32_t* facets)
{
  if (nlist < 0 || (nlist > 0 && !facets))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: nlist = %d, or a null list", who, (int)nlist);
  if (nlist >= FACET_LIST_END) // (2^28: eqlb_facet_plan.h)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: nlist = %d: at most 2^28 - 1 facets", who, (int)nlist);
  return EQLB_OK;
}

// the end of a setter of a facet term, an empty list: the term off, the diagonal formed again
template <class H>
int solver_facet_term_off(H* h, int32_t memspace, hipStream_t stream)
{
  h->facet.on = h->facet.positive = false;
  h->facet.n = 0;
  HIP_TRY(enqueue_diagonal(*h, h->diag, stream));
  if (memspace == EQLB_MEM_HOST)
    HIP_TRY(hipStreamSynchronize(stream));
  return EQLB_OK;
}

// ... and with a plan (FacetTermPlan): its arrays in the place of the old ones, the diagonal formed again.  kw: the
// tensor weights of a spring term (bs = 2), which go in here with the rest, so that nothing of the handle changes before
// this point
template <class H>
int solver_facet_term_commit(H* h, FacetTermPlan& plan, int32_t nlist, bool positive, int32_t memspace,
                             hipStream_t stream, DevBuf<double>* kw = nullptr)
{
  FacetTerm& t = h->facet;
  if (kw)
    t.kw = std::move(*kw);
  t.tab = std::move(plan.tab);
  t.val = std::move(plan.val);
  t.n = nlist;
  t.at = plan.at;
  t.on = true;
  t.positive = positive;
  HIP_TRY(enqueue_diagonal(*h, h->diag, stream));
  if (memspace == EQLB_MEM_HOST)
    HIP_TRY(hipStreamSynchronize(stream));
  return EQLB_OK;
}

// the points of eqlb_primal_robin_flux and eqlb_elasticity_spring_flux, a kernel argument
constexpr int RF_MAX_NQ = 64;
struct FacetRule
{
  double s[RF_MAX_NQ];
};

// A point of a listed facet for the flux kernels, the rule of eqlb_primal_robin_flux (include/eqlb.h): the facet
// parameter sq of the frame of eqlb_facet_points (the facet seen from its one cell, the low local vertex first) becomes
// the parameter of the facet's own frame (0 at the lower node id), sq or 1 - sq, and l[j] the value there of the
// equispaced 1-D Lagrange basis in the facet-local order: the product over the other nodes k, in that order, of
// (s - x_k) / (x_j - x_k) with x = (0, 1, 1/p ... (p-1)/p) formed as j / p, the first factor starts it, every operation
// rounded on its own.  dd: the facet's rows (k_robin_prepare; dd[0] < 0: skipped).  False, and nothing written, for a
// facet the list skipped or whose cell does not hold it; every index is checked before it is used.
__device__ __forceinline__ bool facet_point_basis(int32_t f, const int32_t* dd, double sq, int p, int32_t ncells,
                                                  const int32_t* cell_nodes, const int32_t* cell_facets,
                                                  const int32_t* fco, const int32_t* facet_cells, double* l)
{
#pragma clang fp contract(off)
  int lf = -1;
  int32_t cell = -1;
  if (dd[0] >= 0)
  {
    cell = facet_cells[fco[f]];
    if (cell >= 0 && cell < ncells)
      for (int k = 0; k < 3; ++k)
        if (cell_facets[(int64_t)cell * 3 + k] == f)
          lf = k;
  }
  if (lf < 0)
    return false;
  const int va = (lf == 0) ? 1 : 0, vb = (lf == 2) ? 1 : 2; // the low local vertex first
  const bool same = cell_nodes[(int64_t)cell * 3 + va] < cell_nodes[(int64_t)cell * 3 + vb];
  const double s = same ? sq : 1.0 - sq;
  double xn[PS_PMAX + 1];
  xn[0] = 0.0;
  xn[1] = 1.0;
  for (int j = 1; j < p; ++j)
    xn[1 + j] = (double)j / (double)p;
  for (int j = 0; j <= p; ++j)
  {
    double v = 1.0;
    bool first = true;
    for (int k = 0; k <= p; ++k)
      if (k != j)
      {
        const double fac = (s - xn[k]) / (xn[j] - xn[k]);
        v = first ? fac : v * fac;
        first = false;
      }
    l[j] = v;
  }
  return true;
}

// One thread per (listed facet, point), all BS rows, the kernel of eqlb_primal_robin_flux (BS = 1) and
// eqlb_elasticity_spring_flux (BS = 2): with d_s = u_h,s(x_q) - u_ext[s][i][q] on component s of the blocked u,
//   BS = 1  out[i][q] = alpha_i d_0                              coeff: alpha [nlist]
//   BS = 2  out[r][i][q] = K_i[r][0] d_0 + K_i[r][1] d_1         coeff: K [nlist][3] = (k00, k01, k11)
// The frame and the basis l_j come from facet_point_basis; u_h,s is the sum of l_j u[BS dof_j + s] in ascending j, the
// first product starts it; u_ext is subtracted last; the contraction with K is two products and one addition.  Every
// operation rounded on its own.  A facet the list skipped gives NaN.
template <int BS>
__global__ void __launch_bounds__(PS_THREADS)
k_facet_flux(int32_t nlist, int32_t nq, int32_t p, const FacetRule rule, const int32_t* __restrict__ flist,
             const int32_t* __restrict__ dofs, const double* __restrict__ coeff, int32_t ncells,
             const int32_t* __restrict__ cell_nodes, const int32_t* __restrict__ cell_facets,
             const int32_t* __restrict__ fco, const int32_t* __restrict__ facet_cells, const double* __restrict__ u,
             const double* __restrict__ u_ext, double* __restrict__ out)
{
#pragma clang fp contract(off)
  static_assert(BS == 1 || BS == 2, "a Robin term (BS = 1) or a spring term (BS = 2)");
  const int64_t total = (int64_t)nlist * nq;
  const int64_t t = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (t >= total)
    return;
  const int64_t i = t / nq;
  const int q = (int)(t - i * nq);
  const int32_t* dd = dofs + i * FACET_ROW;
  double l[PS_PMAX + 1];
  if (!facet_point_basis(flist[i], dd, rule.s[q], p, ncells, cell_nodes, cell_facets, fco, facet_cells, l))
  {
    if constexpr (BS == 2)
      out[total + t] = __builtin_nan("");
    out[t] = __builtin_nan("");
    return;
  }
  double d0 = 0.0, d1 = 0.0; // (d1: BS = 2 only)
  for (int j = 0; j <= p; ++j)
  {
    const double p0 = l[j] * u[BS * (int64_t)dd[j]];
    d0 = j == 0 ? p0 : d0 + p0;
    if constexpr (BS == 2)
    {
      const double p1 = l[j] * u[2 * (int64_t)dd[j] + 1];
      d1 = j == 0 ? p1 : d1 + p1;
    }
  }
  if (u_ext)
  {
    d0 = d0 - u_ext[t];
    if constexpr (BS == 2)
      d1 = d1 - u_ext[total + t];
  }
  if constexpr (BS == 1)
    out[t] = coeff[i] * d0;
  else
  {
    const double* k = coeff + 3 * i;
    out[t] = k[0] * d0 + k[1] * d1;
    out[total + t] = k[1] * d0 + k[2] * d1;
  }
}

// the body of eqlb_primal_robin_weights / eqlb_elasticity_spring_weights: *nlist (or nullptr) the listed facets, w
// [capacity >= nlist] rows of one weight (bs = 1) or three (bs = 2) in `memspace`
template <class H>
int solver_facet_weights(const char* who, H* h, int32_t* nlist, double* w, int32_t capacity, int32_t memspace,
                         void* stream_)
{
  EQLB_TRY(check_handle(who, h));
  EQLB_TRY(check_memspace(who, memspace));
  const int32_t n = h->facet.on ? h->facet.n : 0;
  if (nlist)
    *nlist = n;
  if (!w || n == 0)
    return EQLB_OK;
  if (capacity < n)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: capacity = %d is less than the %d listed facets", who, (int)capacity,
                (int)n);
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool host = memspace == EQLB_MEM_HOST;
  HIP_TRY(hipMemcpyAsync(w, facet_weights(*h), (H::bs == 1 ? 1 : 3) * (size_t)n * sizeof(double),
                         host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, stream));
  if (host)
    HIP_TRY(hipStreamSynchronize(stream));
  return EQLB_OK;
}

// the body of eqlb_primal_robin_flux / eqlb_elasticity_spring_flux (k_facet_flux): u [bs ndofs], s HOST [nq], u_ext
// (or nullptr) and out [bs][nlist][nq].  `term` and `setter` name the term and its entry in the message of a handle
// without one
template <class H>
int solver_facet_flux(const char* who, const char* term, const char* setter, H* h, const double* u, int32_t nq,
                      const double* s, const double* u_ext, double* out, int32_t memspace, void* stream_)
{
  EQLB_TRY(check_handle(who, h));
  EQLB_TRY(check_memspace(who, memspace));
  if (!u || !s || !out)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  if (nq < 1 || nq > RF_MAX_NQ)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: nq = %d outside 1 ... %d", who, (int)nq, RF_MAX_NQ);
  FacetRule rule{};
  for (int q = 0; q < nq; ++q)
  {
    if (!(s[q] >= 0.0 && s[q] <= 1.0))
      return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: s[%d] = %g outside [0, 1]", who, q, s[q]);
    rule.s[q] = s[q];
  }
  if (!h->facet.on)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: the handle has no %s term (%s first)", who, term, setter);
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool host = memspace == EQLB_MEM_HOST;
  const DeviceMesh& m = h->mesh->m;
  const size_t np = (size_t)h->facet.n * (size_t)nq, no = H::bs * np;
  HostCall c;
  const auto d_u = c.in(host ? u : nullptr, (size_t)H::bs * h->ndofs);
  const auto d_e = c.in(host ? u_ext : nullptr, no);
  const auto d_o = c.out(host ? out : nullptr, no);
  if (host)
    HIP_TRY(c.upload(stream));
  const int32_t* tab = h->facet.tab.get();
  hipLaunchKernelGGL(k_facet_flux<H::bs>, dim3(grid_of((int64_t)np, PS_THREADS)), dim3(PS_THREADS), 0, stream,
                     h->facet.n, nq, (int32_t)h->p, rule, tab, tab + h->facet.at.dofs, facet_coeffs(*h), m.ncells,
                     m.cell_nodes, m.cell_facets, m.facet_cells_off, m.facet_cells, host ? d_u.get() : u,
                     host ? d_e.get() : u_ext, host ? d_o.get() : out);
  c.note(hipGetLastError());
  HIP_TRY(c.finish(stream));
  return EQLB_OK;
}

// what every *_many entry checks about its column count
inline int check_nrhs(const char* who, int32_t nrhs)
{
  if (nrhs < 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: nrhs = %d (at least 1)", who, (int)nrhs);
  return EQLB_OK;
}

// h: a fresh handle that holds what only its unit knows; cell_coeff [ncells] in `memspace` or nullptr
template <class H>
int solver_create(const char* who, std::unique_ptr<H> h, eqlb_mesh* mesh, int32_t p, const double* cell_coeff,
                  int32_t memspace, void* stream_, H** handle)
{
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
  h->mesh = mesh;
  h->p = p;
  h->nd = nd;
  h->ndofs = ndofs;
  h->has_coeff = cell_coeff != nullptr;
  const size_t nc = (size_t)m.ncells, nslots = 3 * nc * (size_t)(1 + ne), nv = (size_t)H::bs * ndofs;
  h->cell_dofs = h->mem.template piece<int32_t>(nc * nd);
  h->slots = h->mem.template piece<int32_t>(nslots);
  h->status = h->mem.template piece<int32_t>(STATUS_WORDS);
  h->coeff = h->mem.template piece<double>(nc);
  h->yloc = h->mem.template piece<double>(H::bs * nc * nd);
  h->diag = h->mem.template piece<double>(nv);
  h->r = h->mem.template piece<double>(nv);
  h->z = h->mem.template piece<double>(nv);
  h->d = h->mem.template piece<double>(nv);
  h->q = h->mem.template piece<double>(nv);
  h->part = h->mem.template piece<double>(2 * (size_t)PS_MAXBLOCKS);
  h->fixed = h->mem.template piece<uint8_t>(nv);
  h->st = h->mem.template piece<PcgState>(1);
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
  HIP_TRY(hipMemsetAsync(h->status, 0, STATUS_WORDS * sizeof(int32_t), stream));
  HIP_TRY(hipMemsetAsync(h->fixed, 0, nv, stream));
  if (cell_coeff)
    HIP_TRY(hipMemcpyAsync(h->coeff, cell_coeff, nc * sizeof(double),
                           memspace == EQLB_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, stream));
  // the dofmap, by the kernel behind eqlb_mesh_lagrange_dofmap (device memory space: one launch, nothing waits)
  EQLB_TRY(eqlb_mesh_lagrange_dofmap(mesh, p, h->cell_dofs.get(), nullptr, EQLB_MEM_DEVICE, stream_));
  const int64_t nshared = (int64_t)m.nnodes + (int64_t)m.nfacets * ne;
  hipLaunchKernelGGL(k_primal_slots, dim3(grid_of(nshared, PS_THREADS)), dim3(PS_THREADS), 0, stream, s, node_cells,
                     m.facet_cells, h->cell_dofs.get(), h->slots.get(), h->status.get() + (H::bs - 1));
  HIP_TRY(hipGetLastError());
  HIP_TRY(enqueue_diagonal(*h, h->diag, stream));
  if (memspace == EQLB_MEM_HOST)
    HIP_TRY(hipStreamSynchronize(stream)); // (the caller's coefficient array has been read)
  *handle = h.release();
  return EQLB_OK;
}

template <class H>
int solver_ndofs(const char* who, const H* h, int64_t* ndofs)
{
  if (!h || !ndofs)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  *ndofs = h->ndofs;
  return EQLB_OK;
}

// the list of component r is facets[r] [nlist[r]]; the messages name the lists as the unit's entry does: "nlist",
// "facets" for one component, "nlist0", "facets1" for two
template <class H>
int solver_set_dirichlet(const char* who, H* h, const int32_t (&nlist)[H::bs], const int32_t* const (&facets)[H::bs],
                         int32_t memspace, void* stream_)
{
  constexpr int bs = H::bs;
  const char* const tag[2] = {bs == 1 ? "" : "0", "1"};
  for (int r = 0; r < bs; ++r)
    if (nlist[r] < 0 || (nlist[r] > 0 && !facets[r]))
      return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: nlist%s = %d, or a null list", who, tag[r], (int)nlist[r]);
  EQLB_TRY(check_handle(who, h));
  EQLB_TRY(check_memspace(who, memspace));
  const DeviceMesh& m = h->mesh->m;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool host = memspace == EQLB_MEM_HOST;
  if (host)
    for (int r = 0; r < bs; ++r)
      for (int32_t i = 0; i < nlist[r]; ++i)
        if (facets[r][i] < 0 || facets[r][i] >= m.nfacets)
          return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: facets%s[%d] = %d is no facet of the mesh (%d facets)", who, tag[r],
                      (int)i, (int)facets[r][i], (int)m.nfacets);
  HostCall s; // (a device-memory call stages nothing: no allocation, no copy and no wait)
  DevPiece<int32_t> d_f[bs];
  bool any = false;
  for (int r = 0; r < bs; ++r)
  {
    d_f[r] = s.in(host ? facets[r] : nullptr, (size_t)nlist[r]);
    any = any || nlist[r] > 0;
  }
  if (host && any)
    HIP_TRY(s.upload(stream));
  s.note(hipMemsetAsync(h->fixed, 0, (size_t)bs * h->ndofs, stream));
  s.note(hipMemsetAsync(h->status, 0, (1 + bs) * sizeof(int32_t), stream));
  for (int r = 0; r < bs; ++r)
    if (nlist[r] > 0)
    {
      hipLaunchKernelGGL(k_primal_mask<bs>, dim3(grid_of(nlist[r], PS_THREADS)), dim3(PS_THREADS), 0, stream, nlist[r],
                         host ? d_f[r].get() : facets[r], r, m.nnodes, m.nfacets, h->space.ne, m.facet_nodes,
                         h->fixed.get(), h->status.get());
      s.note(hipGetLastError());
    }
  HIP_TRY(s.finish(stream));
  return EQLB_OK;
}

// The setter of the per-cell term d (`term`: its CellTerm in H or the base of H): the array `cell` [ncells][width] in
// `memspace` where given, else the scalar x where the term has one; x == neutral without an array switches the term
// off.  The scalar (only where no array is given; before the handle is read) and a host array are checked before the
// handle changes; an array in device memory is the caller's responsibility.  The diagonal of the handle is formed again
// in place on the stream.
template <class H, class B>
int solver_set_cell_term(const char* who, H* h, const CellTermSpec& d, CellTerm B::*term, double x, const double* cell,
                         int32_t memspace, void* stream_)
{
  EQLB_TRY(check_handle(who, h));
  EQLB_TRY(check_memspace(who, memspace));
  if (!cell && d.scalar)
    EQLB_TRY(check_scalar(who, d.scalar, *d.array.rule, x));
  CellTerm& t = h->*term;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool host = memspace == EQLB_MEM_HOST;
  const size_t nc = (size_t)h->space.ncells, n = nc * d.array.width();
  if (cell && host)
    EQLB_TRY(check_cells(who, (long long)nc, {{d.array, cell}}));
  if (cell)
  {
    if (!t.buf.get())
    {
      const hipError_t e = t.buf.alloc_raw(n);
      if (e != hipSuccess)
        return fail(EQLB_ERR_NO_MEMORY, "%s: device allocation failed: %s", who, hipGetErrorString(e));
    }
    HIP_TRY(hipMemcpyAsync(t.buf.get(), cell, n * sizeof(double), host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice,
                           stream));
  }
  t.cell = cell != nullptr;
  t.scalar = cell ? d.neutral : x;
  t.on = cell != nullptr || x != d.neutral;
  HIP_TRY(enqueue_diagonal(*h, h->diag, stream));
  if (host)
    HIP_TRY(hipStreamSynchronize(stream)); // (the caller's array has been read)
  return EQLB_OK;
}

template <class H>
int solver_load(const char* who, H* h, int32_t degree_dg, const double* rhs_dg, const double* b_extra, double* b,
                int32_t memspace, void* stream_)
{
  if (degree_dg < 0 || degree_dg > PS_DMAX)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: degree_dg = %d outside 0 ... 3", who, (int)degree_dg);
  EQLB_TRY(check_handle(who, h));
  if (!rhs_dg || !b)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  EQLB_TRY(check_memspace(who, memspace));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool host = memspace == EQLB_MEM_HOST;
  const size_t nf = (size_t)H::bs * h->space.ncells * nd_of(degree_dg), n = (size_t)H::bs * h->ndofs;
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

// u, y [nrhs][bs ndofs]: groups of up to max_cols columns, one store pass and one sum pass each
template <class H>
int solver_apply(const char* who, H* h, int32_t nrhs, const double* u, double* y, int32_t masked, int32_t memspace,
                 void* stream_)
{
  EQLB_TRY(check_handle(who, h));
  EQLB_TRY(check_nrhs(who, nrhs));
  if (!u || !y)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  EQLB_TRY(check_memspace(who, memspace));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool host = memspace == EQLB_MEM_HOST;
  const size_t n = (size_t)H::bs * h->ndofs;
  PcgWork w;
  EQLB_TRY(primal_work(h, nrhs < H::max_cols ? nrhs : H::max_cols, w));
  HostCall s;
  const auto d_u = s.in(host ? u : nullptr, nrhs * n);
  const auto d_y = s.out(host ? y : nullptr, nrhs * n);
  if (host)
    HIP_TRY(s.upload(stream));
  const double* pu = host ? d_u.get() : u;
  double* py = host ? d_y.get() : y;
  for (int32_t c0 = 0; c0 < nrhs; c0 += H::max_cols)
  {
    const int R = nrhs - c0 < H::max_cols ? nrhs - c0 : H::max_cols;
    const ManyCols cols{R, (1u << R) - 1u, 0, nullptr};
    s.note(launch_cell<CELL_OPERATOR>(*h, cols, 0, pu + c0 * n, false, stream));
    GatherArgs g = gather_args(*h, cols, masked != 0);
    g.y = py + c0 * n;
    s.note(launch_gather_op(*h, g, pu + c0 * n, false, stream));
  }
  HIP_TRY(s.finish(stream));
  return EQLB_OK;
}

template <class H>
int solver_diagonal(const char* who, H* h, double* out, int32_t memspace, void* stream_)
{
  EQLB_TRY(check_handle(who, h));
  if (!out)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  EQLB_TRY(check_memspace(who, memspace));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool host = memspace == EQLB_MEM_HOST;
  HostCall s;
  const auto d_o = s.out(host ? out : nullptr, (size_t)H::bs * h->ndofs);
  if (host)
    HIP_TRY(s.upload(stream));
  s.note(enqueue_diagonal(*h, host ? d_o.get() : out, stream));
  HIP_TRY(s.finish(stream));
  return EQLB_OK;
}

template <class H>
int solver_residual(const char* who, H* h, const double* b, const double* u, double* r, double* norms, int32_t memspace,
                    void* stream_)
{
  EQLB_TRY(check_handle(who, h));
  if (!b || !u || !r)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  EQLB_TRY(check_memspace(who, memspace));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool host = memspace == EQLB_MEM_HOST;
  const size_t n = (size_t)H::bs * h->ndofs;
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

// b, u [nrhs][bs ndofs], info HOST [nrhs][8]
template <class H>
int solver_solve(const char* who, H* h, int32_t nrhs, const double* b, double* u, double rtol, double atol,
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
  int32_t status[STATUS_WORDS] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(status, h->status.get(), sizeof(status), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  for (int r = 0; r < H::bs; ++r)
    if (status[1 + r] < 1 && !(h->facet.on && h->facet.positive)) // (a facet term with some weight > 0: definite as it is)
    {
      if constexpr (H::bs == 1)
        return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: singular: no Dirichlet DOF (eqlb_primal_set_dirichlet first)", who);
      else
        return fail(EQLB_ERR_INVALID_ARGUMENT,
                    "%s: singular: component %d has no Dirichlet DOF (eqlb_elasticity_set_dirichlet first)", who, r);
    }
  PcgWork grown;
  EQLB_TRY(primal_work(h, nrhs < H::max_cols ? nrhs : H::max_cols, grown));
  auto residual = [&](const ManyCols& c, const double* xb, const double* xu, double* r, bool only_fixed) {
    return enqueue_residual(*h, c, xb, xu, r, only_fixed, stream);
  };
  auto product = [&](const ManyCols& c) { return enqueue_product(*h, c, stream); };
  return pcg_solve_groups(H::bs * h->ndofs, nrhs, b, u, info, memspace == EQLB_MEM_HOST, stream,
                          [&](int R, const double* pb, double* pu, double* pinfo) {
                            const PcgWork w = work_of(*h, R);
                            return pcg_solve(w, residual, product, JacobiSteps<H::max_cols>{w, stream}, pb, pu, rtol,
                                             atol, maxit, pinfo, status[0], stream);
                          });
}
} // namespace
} // namespace eqlb
