// Values of the flux boundary conditions on the device (include/eqlb.h: eqlb_facet_points, eqlb_flux_bc_dofs,
// eqlb_se_update_flux_bc / eqlb_ev_update_flux_bc, eqlb_*_get_boundary_values).  The patch kernels only READ the
// table SeArgs::bvals at run time; bins, tiles, groups of boundary patches and the choice of the launches depend on
// the facet types alone.  So new values of a load step or time step are written into the table in place, one thread
// per listed facet, and nothing of eqlb_se_set_boundary is repeated.  The facet DOFs are those base::BoundaryData
// forms on the host (base/BoundaryData.cpp:470-575; wrappers.cpp, BoundaryData::evaluate):
//   DOF_j = pf_f sign(det J) |E| sum_q w_q g_q s_q^j,   pf_f = +1 for local facet 1, -1 otherwise.
// The lists are O(sqrt(N)) long: the kernels are bound by the launch latency and are not tuned.
#include "eqlb_internal.h"
#include "eqlb_handle.h"

#include <cmath>
#include <cstring>

namespace eqlb
{
constexpr int BC_MAX_NQ = 64, BC_THREADS = 256;

// facet rule, by value in the kernel argument (1 KB): no upload, no synchronisation
struct BcRule
{
  double s[BC_MAX_NQ];
  double w[BC_MAX_NQ];
};

struct BcArgs
{
  int32_t nlist, k, nq, vector;
  int32_t nnodes, ncells, nfacets;
  int32_t rhs;              // row of the table
  int32_t check_only;       // 1: count the refused entries, write nothing
  const int32_t* facets;    // [nlist]
  const double* values;     // nq = 0: [nlist][k] facet DOFs; vector = 0: [nlist][nq]; vector = 1: [nlist][nq][2]
  const double* x;          // mesh
  const int32_t *cell_nodes, *cell_facets, *facet_cells_off, *facet_cells;
  const int8_t* facet_type; // [nfacets] types of the row, or nullptr (mesh-only entry points: any boundary facet)
  double* dofs;             // [nlist][k] or nullptr
  double* bvals;            // [nrhs][ncells*k(k+2)] table of a handle or nullptr
  int32_t* nrejected;       // refused entries (atomic count) or nullptr
  int32_t* first_bad;       // lowest list position of a refused entry (host memory space) or nullptr
};

// The one cell of a boundary facet, the local id of the facet in it and the vertices of the cell.  Every index is
// checked before it is used: false = nothing of the entry may be read or written.
__device__ __forceinline__ bool bc_locate(const BcArgs& a, int32_t fct, int32_t& cell, int& lf, double (&X)[3][2])
{
  if (fct < 0 || fct >= a.nfacets)
    return false;
  const int32_t o0 = a.facet_cells_off[fct];
  if (a.facet_cells_off[fct + 1] - o0 != 1)
    return false;
  cell = a.facet_cells[o0];
  if (cell < 0 || cell >= a.ncells)
    return false;
  lf = -1;
  for (int l = 0; l < 3; ++l)
    if (a.cell_facets[(int64_t)cell * 3 + l] == fct)
      lf = l;
  if (lf < 0)
    return false;
  if (a.facet_type != nullptr && a.facet_type[fct] != EQLB_FACET_ESSNT_DUAL)
    return false;
  for (int v = 0; v < 3; ++v)
  {
    const int32_t nd = a.cell_nodes[(int64_t)cell * 3 + v];
    if (nd < 0 || nd >= a.nnodes)
      return false;
    X[v][0] = a.x[(int64_t)nd * 3];
    X[v][1] = a.x[(int64_t)nd * 3 + 1];
  }
  return true;
}

__device__ __forceinline__ void bc_refuse(const BcArgs& a, int32_t t)
{
  if (a.nrejected)
    atomicAdd(a.nrejected, 1);
  if (a.first_bad)
    atomicMin(a.first_bad, t);
}

// Moments of the listed values.  The k accumulators run over q in ascending order with s^j as a running product, and
// no product is contracted into the following sum: every instance of the kernel (moments alone, moments + scatter)
// gives the same bits.
__device__ __forceinline__ void bc_moments(const BcArgs& a, const BcRule& rule, int32_t t, int lf,
                                           const double (&X)[3][2], double (&dof)[4])
{
#pragma clang fp contract(off)
  const double j00 = X[1][0] - X[0][0], j01 = X[2][0] - X[0][0];
  const double j10 = X[1][1] - X[0][1], j11 = X[2][1] - X[0][1];
  const double det = j00 * j11 - j01 * j10; // sign(det J) from the vertices: no handle, no cellJ
  const int va = (lf == 0) ? 1 : 0, vb = (lf == 2) ? 1 : 2; // the low local vertex first
  const double ex = X[vb][0] - X[va][0], ey = X[vb][1] - X[va][1];
  const double scale = ((lf == 1) ? 1.0 : -1.0) * ((det > 0.0) ? 1.0 : -1.0) * sqrt(ex * ex + ey * ey);
  double nx = 0.0, ny = 0.0;
  if (a.vector)
  {
    // outward unit normal: away from the vertex opposite the facet
    const double h = hypot(ex, ey);
    nx = ey / h;
    ny = -ex / h;
    if (nx * (X[lf][0] - X[va][0]) + ny * (X[lf][1] - X[va][1]) > 0.0)
    {
      nx = -nx;
      ny = -ny;
    }
  }
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int q = 0; q < a.nq; ++q)
  {
    double g;
    if (a.vector)
    {
      const double* v = a.values + ((int64_t)t * a.nq + q) * 2;
      g = v[0] * nx + v[1] * ny;
    }
    else
      g = a.values[(int64_t)t * a.nq + q];
    const double wg = rule.w[q] * g, s = rule.s[q];
    double sp = 1.0;
    for (int j = 0; j < a.k; ++j)
    {
      acc[j] = acc[j] + wg * sp;
      sp = sp * s;
    }
  }
  for (int j = 0; j < a.k; ++j)
    dof[j] = scale * acc[j];
}

// One thread per listed facet: facet DOFs from point values (nq >= 1) or as given (nq = 0), written to dofs and / or
// into the table of a handle.  A refused entry writes nothing into the table; the mesh-only call (no table) marks its
// row of dofs with NaN.
__global__ void __launch_bounds__(BC_THREADS) k_flux_bc(const BcArgs a, const BcRule rule)
{
  const int32_t t = blockIdx.x * BC_THREADS + threadIdx.x;
  if (t >= a.nlist)
    return;
  int32_t cell = -1;
  int lf = -1;
  double X[3][2];
  if (!bc_locate(a, a.facets[t], cell, lf, X))
  {
    bc_refuse(a, t);
    if (a.dofs && !a.check_only)
      for (int j = 0; j < a.k; ++j)
        a.dofs[(int64_t)t * a.k + j] = __builtin_nan("");
    return;
  }
  if (a.check_only)
    return;
  double dof[4] = {0.0, 0.0, 0.0, 0.0};
  if (a.nq == 0)
    for (int j = 0; j < a.k; ++j)
      dof[j] = a.values[(int64_t)t * a.k + j];
  else
    bc_moments(a, rule, t, lf, X, dof);
  if (a.dofs)
    for (int j = 0; j < a.k; ++j)
      a.dofs[(int64_t)t * a.k + j] = dof[j];
  if (a.bvals)
  {
    const int nrt = a.k * (a.k + 2);
    double* row = a.bvals + ((int64_t)a.rhs * a.ncells + cell) * nrt + lf * a.k;
    for (int j = 0; j < a.k; ++j)
      row[j] = dof[j];
  }
}

// xq [nlist][nq][2]: x0 + J X with the reference point X of the facet parameter (eqlb/bcs.py, _facet_points)
__global__ void __launch_bounds__(BC_THREADS) k_facet_points(const BcArgs a, const BcRule rule, double* __restrict__ xq)
{
#pragma clang fp contract(off)
  const int32_t t = blockIdx.x * BC_THREADS + threadIdx.x;
  if (t >= a.nlist)
    return;
  int32_t cell = -1;
  int lf = -1;
  double X[3][2];
  double* out = xq + (int64_t)t * a.nq * 2;
  if (!bc_locate(a, a.facets[t], cell, lf, X))
  {
    for (int q = 0; q < 2 * a.nq; ++q)
      out[q] = __builtin_nan("");
    return;
  }
  const double j00 = X[1][0] - X[0][0], j01 = X[2][0] - X[0][0];
  const double j10 = X[1][1] - X[0][1], j11 = X[2][1] - X[0][1];
  for (int q = 0; q < a.nq; ++q)
  {
    const double s = rule.s[q];
    const double Xr = (lf == 0) ? 1.0 - s : ((lf == 1) ? 0.0 : s);
    const double Yr = (lf == 2) ? 0.0 : s;
    out[2 * q] = X[0][0] + (Xr * j00 + Yr * j01);
    out[2 * q + 1] = X[0][1] + (Xr * j10 + Yr * j11);
  }
}

} // namespace eqlb

namespace
{
using eqlb::BcArgs;
using eqlb::BcRule;

BcArgs mesh_args(const eqlb::DeviceMesh& m, int32_t nlist, const int32_t* facets)
{
  BcArgs a{};
  a.nlist = nlist;
  a.nnodes = m.nnodes;
  a.ncells = m.ncells;
  a.nfacets = m.nfacets;
  a.facets = facets;
  a.x = m.x;
  a.cell_nodes = m.cell_nodes;
  a.cell_facets = m.cell_facets;
  a.facet_cells_off = m.facet_cells_off;
  a.facet_cells = m.facet_cells;
  return a;
}

// the checks every entry point makes before any device call
int check_rule(const char* who, int32_t nq, int32_t nq_min, const double* s, const double* w, bool need_w)
{
  if (nq < nq_min || nq > eqlb::BC_MAX_NQ)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: nq = %d outside %d ... %d", who, (int)nq, (int)nq_min, eqlb::BC_MAX_NQ);
  if (nq > 0 && (!s || (need_w && !w)))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: the facet rule is a null pointer", who);
  for (int32_t q = 0; q < nq; ++q)
    if (!(s[q] >= 0.0 && s[q] <= 1.0))
      return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: s[%d] = %g outside [0, 1]", who, (int)q, s[q]);
  return EQLB_OK;
}

void fill_rule(BcRule& r, int32_t nq, const double* s, const double* w)
{
  std::memset(&r, 0, sizeof(r));
  for (int32_t q = 0; q < nq; ++q)
  {
    r.s[q] = s[q];
    r.w[q] = w ? w[q] : 0.0;
  }
}

// host memory space of the mesh-only entry points: the listed facets are boundary facets of the mesh
int check_boundary_facets(const char* who, const eqlb_mesh* mesh, int32_t nlist, const int32_t* facets)
{
  const std::vector<int32_t>& off = mesh->host.facet_cells_off;
  for (int32_t i = 0; i < nlist; ++i)
  {
    const int32_t f = facets[i];
    if (f < 0 || f >= mesh->m.nfacets)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: facets[%d] = %d is no facet of the mesh", who, (int)i, (int)f);
    if (off[(size_t)f + 1] - off[f] != 1)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: facets[%d] = %d lies between two cells", who, (int)i, (int)f);
  }
  return EQLB_OK;
}

size_t values_count(int32_t nlist, int32_t k, int32_t nq, int32_t vector)
{
  return (nq == 0) ? (size_t)nlist * k : (size_t)nlist * nq * (vector ? 2 : 1);
}

inline void launch_flux_bc(const BcArgs& a, const BcRule& rule, hipStream_t stream)
{
  hipLaunchKernelGGL(eqlb::k_flux_bc, dim3((a.nlist + eqlb::BC_THREADS - 1) / eqlb::BC_THREADS),
                     dim3(eqlb::BC_THREADS), 0, stream, a, rule);
}

int update_flux_bc(const char* who, eqlb_se* h, int32_t rhs, int32_t nlist, const int32_t* facets, int32_t nq,
                   const double* s, const double* w, const double* values, int32_t vector, int32_t* nrejected,
                   int32_t memspace, void* stream_)
{
  // (the arguments that need no handle first: each refusal has a message of its own)
  if (nlist < 0 || (nlist > 0 && (!facets || !values)))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: invalid list (nlist = %d)", who, (int)nlist);
  if (vector != 0 && vector != 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: vector must be 0 or 1", who);
  EQLB_TRY(eqlb::check_memspace(who, memspace));
  EQLB_TRY(check_rule(who, nq, 0, s, w, true));
  if (!h)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null handle", who);
  if (rhs < 0 || rhs >= h->nrhs)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: right-hand side %d outside 0 ... %d", who, (int)rhs, h->nrhs - 1);
  if (!h->bt.boundary_set)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: boundary data not set (no accepted eqlb_%s_set_boundary)", who,
                h->mode == 1 ? "ev" : "se");
  const eqlb::DeviceMesh& m = h->mesh->m;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  BcRule rule;
  fill_rule(rule, nq, s, w);
  BcArgs a = mesh_args(m, nlist, facets);
  a.k = h->k;
  a.nq = nq;
  a.vector = vector;
  a.rhs = rhs;
  a.values = values;
  a.facet_type = h->bt.facet_type + (size_t)rhs * m.nfacets;
  const size_t ntable = (size_t)h->nrhs * m.ncells * h->nrt;
  // a handle with homogeneous values has no table: the first update allocates it, zero-filled, ordered on the stream
  auto ensure_table = [&]() -> int {
    if (h->bt.bvals)
      return EQLB_OK;
    if (h->bt.bvals.alloc(ntable))
      return EQLB_ERR_DEVICE;
    HIP_TRY(hipMemsetAsync(h->bt.bvals, 0, sizeof(double) * ntable, stream));
    return EQLB_OK;
  };
  if (memspace == EQLB_MEM_DEVICE)
  {
    if (nrejected)
      HIP_TRY(hipMemsetAsync(nrejected, 0, sizeof(int32_t), stream));
    if (nlist == 0)
      return EQLB_OK;
    EQLB_TRY(ensure_table());
    a.bvals = h->bt.bvals;
    a.nrejected = nrejected;
    launch_flux_bc(a, rule, stream);
    HIP_TRY(hipGetLastError());
    return EQLB_OK;
  }
  if (nrejected)
    *nrejected = 0;
  if (nlist == 0)
    return EQLB_OK;
  // host memory space: a pass that only checks the list, then the pass that writes - a refused list leaves the table
  // as it was
  const int32_t cnt_init[2] = {0, INT32_MAX};
  int32_t cnt[2] = {0, 0};
  eqlb::HostCall st;
  const auto d_facets = st.in(facets, (size_t)nlist);
  const auto d_values = st.in(values, values_count(nlist, h->k, nq, vector));
  const auto d_cnt = st.in(cnt_init, 2); // rejected facets, first of them
  st.out_prefix(cnt, d_cnt, 2);
  HIP_TRY(st.upload(stream));
  a.facets = d_facets;
  a.values = d_values;
  a.nrejected = d_cnt;
  a.first_bad = d_cnt + 1;
  a.check_only = 1;
  launch_flux_bc(a, rule, stream);
  HIP_TRY(st.finish(stream));
  if (cnt[0] > 0)
  {
    const int32_t i = cnt[1], f = facets[i];
    if (nrejected)
      *nrejected = cnt[0];
    if (f < 0 || f >= m.nfacets)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: facets[%d] = %d is no facet of the mesh", who, (int)i, (int)f);
    const std::vector<int32_t>& off = h->mesh->host.facet_cells_off;
    if (off[(size_t)f + 1] - off[f] != 1)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: facets[%d] = %d lies between two cells: no flux boundary condition",
                  who, (int)i, (int)f);
    return fail(EQLB_ERR_INVALID_ARGUMENT,
                "%s: facets[%d] = %d has no flux boundary condition (type EQLB_FACET_ESSNT_DUAL) on right-hand side %d",
                who, (int)i, (int)f, (int)rhs);
  }
  EQLB_TRY(ensure_table());
  a.bvals = h->bt.bvals;
  a.nrejected = nullptr;
  a.first_bad = nullptr;
  a.check_only = 0;
  launch_flux_bc(a, rule, stream);
  st.note(hipGetLastError());
  HIP_TRY(st.finish(stream));
  return EQLB_OK;
}

int get_boundary_values(const char* who, eqlb_se* h, double* out, int32_t memspace, void* stream_)
{
  if (!h || !out)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  EQLB_TRY(eqlb::check_memspace(who, memspace));
  if (!h->bt.boundary_set)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: boundary data not set", who);
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const size_t bytes = sizeof(double) * (size_t)h->nrhs * h->mesh->m.ncells * h->nrt;
  if (memspace == EQLB_MEM_DEVICE)
  {
    if (h->bt.bvals)
      HIP_TRY(hipMemcpyAsync(out, h->bt.bvals, bytes, hipMemcpyDeviceToDevice, stream));
    else
      HIP_TRY(hipMemsetAsync(out, 0, bytes, stream));
    return EQLB_OK;
  }
  if (!h->bt.bvals)
  {
    std::memset(out, 0, bytes);
    return EQLB_OK;
  }
  HIP_TRY(hipMemcpyAsync(out, h->bt.bvals, bytes, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return EQLB_OK;
}
} // namespace

extern "C" {

int eqlb_facet_points(eqlb_mesh_t* mesh, int32_t nlist, const int32_t* facets, int32_t nq, const double* s,
                      double* xq, int32_t memspace, void* stream_)
try
{
  const char* who = "eqlb_facet_points";
  if (nlist < 0 || (nlist > 0 && (!facets || !xq)))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: invalid list (nlist = %d)", who, (int)nlist);
  EQLB_TRY(eqlb::check_memspace(who, memspace));
  EQLB_TRY(check_rule(who, nq, 1, s, nullptr, false));
  if (!mesh)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null mesh", who);
  const eqlb::DeviceMesh& m = mesh->m;
  if (memspace == EQLB_MEM_HOST)
    EQLB_TRY(check_boundary_facets(who, mesh, nlist, facets));
  if (nlist == 0)
    return EQLB_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  BcRule rule;
  fill_rule(rule, nq, s, nullptr);
  BcArgs a = mesh_args(m, nlist, facets);
  a.nq = nq;
  const dim3 grid((nlist + eqlb::BC_THREADS - 1) / eqlb::BC_THREADS), block(eqlb::BC_THREADS);
  if (memspace == EQLB_MEM_DEVICE)
  {
    hipLaunchKernelGGL(eqlb::k_facet_points, grid, block, 0, stream, a, rule, xq);
    HIP_TRY(hipGetLastError());
    return EQLB_OK;
  }
  eqlb::HostCall st;
  const auto d_facets = st.in(facets, (size_t)nlist);
  const auto d_xq = st.out(xq, (size_t)nlist * nq * 2);
  HIP_TRY(st.upload(stream));
  a.facets = d_facets;
  hipLaunchKernelGGL(eqlb::k_facet_points, grid, block, 0, stream, a, rule, d_xq.get());
  st.note(hipGetLastError());
  HIP_TRY(st.finish(stream));
  return EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_flux_bc_dofs(eqlb_mesh_t* mesh, int32_t k, int32_t nlist, const int32_t* facets, int32_t nq, const double* s,
                      const double* w, const double* values, int32_t vector, double* dofs, int32_t memspace,
                      void* stream_)
try
{
  const char* who = "eqlb_flux_bc_dofs";
  if (k < 1 || k > 4)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: flux degree k = %d outside 1 ... 4", who, (int)k);
  if (nlist < 0 || (nlist > 0 && (!facets || !values || !dofs)))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: invalid list (nlist = %d)", who, (int)nlist);
  if (vector != 0 && vector != 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: vector must be 0 or 1", who);
  EQLB_TRY(eqlb::check_memspace(who, memspace));
  EQLB_TRY(check_rule(who, nq, 1, s, w, true));
  if (!mesh)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null mesh", who);
  const eqlb::DeviceMesh& m = mesh->m;
  if (memspace == EQLB_MEM_HOST)
    EQLB_TRY(check_boundary_facets(who, mesh, nlist, facets));
  if (nlist == 0)
    return EQLB_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  BcRule rule;
  fill_rule(rule, nq, s, w);
  BcArgs a = mesh_args(m, nlist, facets);
  a.k = k;
  a.nq = nq;
  a.vector = vector;
  a.values = values;
  a.dofs = dofs;
  if (memspace == EQLB_MEM_DEVICE)
  {
    launch_flux_bc(a, rule, stream);
    HIP_TRY(hipGetLastError());
    return EQLB_OK;
  }
  eqlb::HostCall st;
  const auto d_facets = st.in(facets, (size_t)nlist);
  const auto d_values = st.in(values, values_count(nlist, k, nq, vector));
  const auto d_dofs = st.out(dofs, (size_t)nlist * k);
  HIP_TRY(st.upload(stream));
  a.facets = d_facets;
  a.values = d_values;
  a.dofs = d_dofs;
  launch_flux_bc(a, rule, stream);
  st.note(hipGetLastError());
  HIP_TRY(st.finish(stream));
  return EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_se_update_flux_bc(eqlb_se_t* h, int32_t rhs, int32_t nlist, const int32_t* facets, int32_t nq,
                           const double* s, const double* w, const double* values, int32_t vector,
                           int32_t* nrejected, int32_t memspace, void* stream)
try
{
  return update_flux_bc("eqlb_se_update_flux_bc", h, rhs, nlist, facets, nq, s, w, values, vector, nrejected, memspace,
                        stream);
}
EQLB_CATCH_ALL

int eqlb_ev_update_flux_bc(eqlb_ev_t* h, int32_t rhs, int32_t nlist, const int32_t* facets, int32_t nq,
                           const double* s, const double* w, const double* values, int32_t vector,
                           int32_t* nrejected, int32_t memspace, void* stream)
try
{
  return update_flux_bc("eqlb_ev_update_flux_bc", h ? h->se.get() : nullptr, rhs, nlist, facets, nq, s, w, values, vector,
                        nrejected, memspace, stream);
}
EQLB_CATCH_ALL

int eqlb_se_get_boundary_values(eqlb_se_t* h, double* out, int32_t memspace, void* stream)
{
  return get_boundary_values("eqlb_se_get_boundary_values", h, out, memspace, stream);
}

int eqlb_ev_get_boundary_values(eqlb_ev_t* h, double* out, int32_t memspace, void* stream)
{
  return get_boundary_values("eqlb_ev_get_boundary_values", h ? h->se.get() : nullptr, out, memspace, stream);
}

} // extern "C"
