// Boundary conditions of the equilibrator across one refinement level ON THE DEVICE (include/eqlb.h:
// eqlb_refine_facet_types, eqlb_refine_child_facets, eqlb_refine_prolong_flux_bc, eqlb_se_carry_boundary /
// eqlb_ev_carry_boundary).  The rule is stated in include/eqlb.h and, as numpy, in dolfinx_eqlb_amd/mesh/refine.py
// (carry_facet_types, child_facets) and mesh/transfer.py (prolong_flux_bc); the device reproduces the numpy statement
// bit for bit.
//
// Children keep the orientation of their parent and a boundary facet of the refined mesh is a whole parent facet or
// one of its halves, so the k facet DOFs of a child (moments of the normal flux) are one of six fixed k x k matrices
// (tools/gen_tables.py: FluxBcProlong<k>, exact rationals) applied to those of the parent: the facet length cancels,
// no coordinates are read.
//
//   k_carry_facet_types   one thread per facet of the refined handle: the type of parent_facet_of, all rows
//   k_child_facets        one thread per listed OLD facet: its one or two children, looked up among the facets of the
//                         low node in the refined handle (as k_find_facets does)
//   k_prolong_flux_bc<K>  one thread per listed facet of the refined handle (dofs rows), or per facet of the refined
//                         handle with the type ESSNT_DUAL (table to table: eqlb_*_carry_boundary), all rows
// The lists are O(sqrt(N)) long and the work per thread is a handful of integer gathers and a k x k product: the
// kernels are bound by the launch latency and are not tuned.  Every facet, cell and node index is checked before it
// addresses anything; the only atomic is atomicMin on the refusal word of a host-memory call.  The parent cell of a
// child comes from a bisection of coff (the plan keeps no parent table).
#include "eqlb_handle.h"
#include "eqlb_refine_device.h"
#include "eqlb_refine_plan.h"
#include "eqlb_tables_gen.h"

#include <climits>

namespace eqlb
{
namespace
{
constexpr int CB_THREADS = 256;

struct CarryArgs
{
  // the old mesh and the plan
  int32_t nnodes, ncells, nfacets, nbis;
  const int32_t *cell_nodes, *cell_facets, *facet_nodes, *node_facets_off, *node_facets;
  const int32_t *bis_facet, *fE, *frank;
  const uint32_t* coff;
  // the refined handle
  int32_t nnodes2, ncells2, nfacets2;
  const int32_t *cell_nodes2, *cell_facets2, *facet_nodes2, *facet_cells_off2, *facet_cells2;
  const int32_t *node_facets_off2, *node_facets2;
  // the call
  int32_t nrhs, nlist;
  const int32_t* list;        // [nlist] facet ids, or nullptr: every facet of the refined handle
  const int8_t *ft, *ft2;     // [nrhs][nfacets], [nrhs][nfacets2]
  int8_t* ft2_out;
  int32_t* children;          // [nlist][2]
  const double* bvals;        // [nrhs][ncells * k(k+2)]
  double* dofs;               // [nrhs][nlist][k] or nullptr
  double* bvals2;             // [nrhs][ncells2 * k(k+2)] or nullptr
  int32_t* first_bad;         // lowest list position of a refused entry (check pass of a host-memory call) or nullptr
};

__global__ void __launch_bounds__(CB_THREADS) k_carry_facet_types(const CarryArgs a)
{
  const int32_t f2 = blockIdx.x * CB_THREADS + threadIdx.x;
  if (f2 >= a.nfacets2)
    return;
  const int32_t p = parent_facet_of(f2, a.nnodes, a.facet_nodes2, a.bis_facet, a.facet_nodes, a.node_facets_off,
                                    a.node_facets);
  const bool has = p >= 0 && p < a.nfacets;
  for (int r = 0; r < a.nrhs; ++r)
    a.ft2_out[(int64_t)r * a.nfacets2 + f2] = has ? a.ft[(int64_t)r * a.nfacets + p] : (int8_t)EQLB_FACET_INTERNAL;
}

// facet of the refined handle with the nodes (n0, n1) in either order, -1 if there is none
__device__ __forceinline__ int32_t find_facet2(const CarryArgs& a, int32_t n0, int32_t n1)
{
  int32_t found = -1;
  if (n0 >= 0 && n0 < a.nnodes2 && n1 >= 0 && n1 < a.nnodes2)
    for (int32_t q = a.node_facets_off2[n0]; q < a.node_facets_off2[n0 + 1] && found < 0; ++q)
    {
      const int32_t f = a.node_facets2[q];
      if (f < 0 || f >= a.nfacets2)
        continue;
      const int32_t m0 = a.facet_nodes2[2 * (int64_t)f], m1 = a.facet_nodes2[2 * (int64_t)f + 1];
      if ((m0 == n0 && m1 == n1) || (m0 == n1 && m1 == n0))
        found = f;
    }
  return found;
}

__global__ void __launch_bounds__(CB_THREADS) k_child_facets(const CarryArgs a)
{
  const int32_t t = blockIdx.x * CB_THREADS + threadIdx.x;
  if (t >= a.nlist)
    return;
  const int32_t f = a.list[t];
  int32_t c0 = -1, c1 = -1;
  if (f >= 0 && f < a.nfacets)
  {
    const int32_t n0 = a.facet_nodes[2 * (int64_t)f], n1 = a.facet_nodes[2 * (int64_t)f + 1];
    const int32_t lo = n0 < n1 ? n0 : n1, hi = n0 < n1 ? n1 : n0;
    if (a.fE[f])
    {
      const int32_t rank = a.frank[f];
      if (rank >= 0 && rank < a.nbis)
      {
        const int32_t m = a.nnodes + rank;
        c0 = find_facet2(a, lo, m);
        c1 = find_facet2(a, m, hi);
      }
    }
    else
      c0 = find_facet2(a, lo, hi);
  }
  a.children[2 * (int64_t)t] = c0;
  a.children[2 * (int64_t)t + 1] = c1;
}

// Where a boundary facet f2 of the refined handle sits: its one cell c2 and local index l2 there, the parent cell c
// and the local index l of the parent facet there, the map m of the facet parameter (0 ... 5, the order of
// FluxBcProlong).  false: the facet is out of range, lies between two cells, has no parent, or the handle is not the
// refined mesh of the plan - nothing out of range has been read.
__device__ __forceinline__ bool carry_locate(const CarryArgs& a, int32_t f2, int32_t& c2, int& l2, int32_t& c, int& l,
                                             int& m)
{
  if (f2 < 0 || f2 >= a.nfacets2)
    return false;
  const int32_t o = a.facet_cells_off2[f2];
  if (a.facet_cells_off2[f2 + 1] - o != 1)
    return false;
  c2 = a.facet_cells2[o];
  if (c2 < 0 || c2 >= a.ncells2)
    return false;
  l2 = -1;
  for (int j = 0; j < 3; ++j)
    if (a.cell_facets2[3 * (int64_t)c2 + j] == f2)
      l2 = j;
  if (l2 < 0)
    return false;
  const int32_t pf = parent_facet_of(f2, a.nnodes, a.facet_nodes2, a.bis_facet, a.facet_nodes, a.node_facets_off,
                                     a.node_facets);
  if (pf < 0 || pf >= a.nfacets)
    return false;
  // the parent: the last cell whose first child is not behind c2 (coff ascends, coff[0] = 0, coff[ncells] = ncells2)
  int32_t lo = 0, hi = a.ncells;
  while (hi - lo > 1)
  {
    const int32_t mid = lo + (hi - lo) / 2;
    if (a.coff[mid] <= (uint32_t)c2)
      lo = mid;
    else
      hi = mid;
  }
  c = lo;
  if (!(a.coff[c] <= (uint32_t)c2 && (uint32_t)c2 < a.coff[c + 1]))
    return false;
  l = -1;
  for (int j = 0; j < 3; ++j)
    if (a.cell_facets[3 * (int64_t)c + j] == pf)
      l = j;
  if (l < 0)
    return false;
  const int va2 = (l2 == 0) ? 1 : 0, vb2 = (l2 == 2) ? 1 : 2, va = (l == 0) ? 1 : 0, vb = (l == 2) ? 1 : 2;
  const int32_t pa = a.cell_nodes[3 * (int64_t)c + va], pb = a.cell_nodes[3 * (int64_t)c + vb];
  // position on the parent facet in half units: 0 the parent's va node, 2 its vb node, 1 the node that bisects it
  auto position = [&](int32_t n) {
    if (n == pa)
      return 0;
    if (n == pb)
      return 2;
    if (n >= a.nnodes && n - a.nnodes < a.nbis && a.bis_facet[n - a.nnodes] == pf)
      return 1;
    return -1;
  };
  const int pos_a = position(a.cell_nodes2[3 * (int64_t)c2 + va2]);
  const int pos_b = position(a.cell_nodes2[3 * (int64_t)c2 + vb2]);
  if (pos_a < 0 || pos_b < 0 || pos_a == pos_b)
    return false;
  // (0,2) (2,0) (0,1) (1,2) (1,0) (2,1)
  if (pos_a == 0)
    m = (pos_b == 2) ? 0 : 2;
  else if (pos_a == 2)
    m = (pos_b == 0) ? 1 : 5;
  else
    m = (pos_b == 2) ? 3 : 4;
  return true;
}

// One thread per listed facet (a.list) or per facet of the refined handle (a.list == nullptr: those of the type
// ESSNT_DUAL in a.ft2 are carried into the table a.bvals2).
template <int K>
__global__ void __launch_bounds__(CB_THREADS) k_prolong_flux_bc(const CarryArgs a)
{
#pragma clang fp contract(off) // the statement rounds every product and every sum on its own
  constexpr int NRT = K * (K + 2);
  const int32_t t = blockIdx.x * CB_THREADS + threadIdx.x;
  if (t >= a.nlist)
    return;
  const int32_t f2 = a.list ? a.list[t] : t;
  if (!a.list)
  {
    bool any = false;
    for (int r = 0; r < a.nrhs; ++r)
      any = any || a.ft2[(int64_t)r * a.nfacets2 + f2] == EQLB_FACET_ESSNT_DUAL;
    if (!any)
      return;
  }
  int32_t c2 = -1, c = -1;
  int l2 = -1, l = -1, m = 0;
  const bool ok = carry_locate(a, f2, c2, l2, c, l, m);
  if (a.first_bad)
  {
    if (!ok)
      atomicMin(a.first_bad, t);
    return;
  }
  const double bad = __longlong_as_double(0x7ff8000000000000ll);
  const double sigma = ((l2 == 1) ? 1.0 : -1.0) * ((l == 1) ? 1.0 : -1.0);
  const double* T = eqlb_tables::FluxBcProlong<K>::FB + (ok ? m : 0) * K * K;
  for (int r = 0; r < a.nrhs; ++r)
  {
    double* dst = nullptr;
    if (a.list)
      dst = a.dofs + ((int64_t)r * a.nlist + t) * K;
    else if (a.ft2[(int64_t)r * a.nfacets2 + f2] == EQLB_FACET_ESSNT_DUAL && c2 >= 0 && c2 < a.ncells2 && l2 >= 0)
      dst = a.bvals2 + ((int64_t)r * a.ncells2 + c2) * NRT + l2 * K;
    if (!dst)
      continue;
    double d[K];
#pragma unroll
    for (int i = 0; i < K; ++i)
      d[i] = ok ? a.bvals[((int64_t)r * a.ncells + c) * NRT + l * K + i] : 0.0;
#pragma unroll
    for (int j = 0; j < K; ++j)
    {
      double s = T[j * K] * d[0];
#pragma unroll
      for (int i = 1; i < K; ++i)
        s = s + T[j * K + i] * d[i];
      dst[j] = ok ? sigma * s : bad;
    }
  }
}

void launch_prolong_flux_bc(int k, const CarryArgs& a, hipStream_t stream)
{
  const dim3 grid(grid_of(a.nlist, CB_THREADS)), block(CB_THREADS);
  switch (k)
  {
  case 1:
    hipLaunchKernelGGL(k_prolong_flux_bc<1>, grid, block, 0, stream, a);
    break;
  case 2:
    hipLaunchKernelGGL(k_prolong_flux_bc<2>, grid, block, 0, stream, a);
    break;
  case 3:
    hipLaunchKernelGGL(k_prolong_flux_bc<3>, grid, block, 0, stream, a);
    break;
  default:
    hipLaunchKernelGGL(k_prolong_flux_bc<4>, grid, block, 0, stream, a);
  }
}

// the arguments every entry shares, after the check of the refined handle every entry makes
int carry_args(const char* who, const eqlb_refine* plan, const eqlb_mesh* refined, CarryArgs& a)
{
  const DeviceMesh &m = plan->mesh->m, &r = refined->m;
  if (r.nnodes != plan->nnodes + plan->nbis || r.ncells != plan->ncells2)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: the handle has %d nodes and %d cells, the refined mesh %d and %d", who,
                r.nnodes, r.ncells, plan->nnodes + plan->nbis, plan->ncells2);
  a = CarryArgs{};
  a.nnodes = plan->nnodes;
  a.ncells = plan->ncells;
  a.nfacets = plan->nfacets;
  a.nbis = plan->nbis;
  a.cell_nodes = m.cell_nodes;
  a.cell_facets = m.cell_facets;
  a.facet_nodes = m.facet_nodes;
  a.node_facets_off = m.node_facets_off;
  a.node_facets = m.node_facets;
  a.bis_facet = plan->bis_facet.get();
  a.fE = plan->fE.get();
  a.frank = plan->frank.get();
  a.coff = plan->coff.get();
  a.nnodes2 = r.nnodes;
  a.ncells2 = r.ncells;
  a.nfacets2 = r.nfacets;
  a.cell_nodes2 = r.cell_nodes;
  a.cell_facets2 = r.cell_facets;
  a.facet_nodes2 = r.facet_nodes;
  a.facet_cells_off2 = r.facet_cells_off;
  a.facet_cells2 = r.facet_cells;
  a.node_facets_off2 = r.node_facets_off;
  a.node_facets2 = r.node_facets;
  return EQLB_OK;
}

const double* flux_bc_table(int k)
{
  return k == 1 ? eqlb_tables::FluxBcProlong<1>::FB
                : k == 2 ? eqlb_tables::FluxBcProlong<2>::FB
                         : k == 3 ? eqlb_tables::FluxBcProlong<3>::FB : eqlb_tables::FluxBcProlong<4>::FB;
}

int carry_boundary(const char* who, const char* kind, const eqlb_se* old, eqlb_refine* plan, eqlb_se* fresh,
                   eqlb_ev* fresh_ev, const uint8_t* node_mask2, void* stream_)
{
  if (!old || !plan || !fresh)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  if (!old->bt.boundary_set)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: the old handle has no boundary data (no accepted eqlb_%s_set_boundary)",
                who, kind);
  if (old->k != fresh->k || old->nrhs != fresh->nrhs || old->stress != fresh->stress)
    return fail(EQLB_ERR_INVALID_ARGUMENT,
                "%s: the handles differ: k = %d and %d, nrhs = %d and %d, stress = %d and %d", who, old->k, fresh->k,
                old->nrhs, fresh->nrhs, old->stress, fresh->stress);
  if (old->mesh != plan->mesh)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: the mesh of the old handle is not the mesh of the plan", who);
  CarryArgs a;
  EQLB_TRY(carry_args(who, plan, fresh->mesh, a));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const int nrhs = old->nrhs, k = old->k;
  const size_t ntypes2 = (size_t)nrhs * a.nfacets2;
  // the types: gathered on the device, copied to the host for the planner of eqlb_se_set_boundary
  std::vector<int8_t> types2(ntypes2);
  {
    DevBuf<int8_t> d_types2;
    EQLB_TRY(d_types2.alloc(ntypes2));
    a.nrhs = nrhs;
    a.ft = old->bt.facet_type;
    a.ft2_out = d_types2.get();
    hipLaunchKernelGGL(k_carry_facet_types, dim3(grid_of(a.nfacets2, CB_THREADS)), dim3(CB_THREADS), 0, stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(types2.data(), d_types2.get(), ntypes2, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
  }
  if (fresh_ev)
    EQLB_TRY(eqlb_ev_set_boundary(fresh_ev, types2.data(), nullptr, node_mask2));
  else
    EQLB_TRY(eqlb_se_set_boundary(fresh, types2.data(), nullptr, node_mask2));
  if (!old->bt.bvals)
    return EQLB_OK; // homogeneous values: the new handle owns no table either
  // the values, from table to table: the new table as the first eqlb_se_update_flux_bc allocates it
  const size_t ntable2 = (size_t)nrhs * a.ncells2 * fresh->nrt;
  if (fresh->bt.bvals.alloc(ntable2))
    return EQLB_ERR_DEVICE;
  HIP_TRY(hipMemsetAsync(fresh->bt.bvals, 0, sizeof(double) * ntable2, stream));
  a.ft2_out = nullptr;
  a.ft2 = fresh->bt.facet_type;
  a.nlist = a.nfacets2;
  a.list = nullptr;
  a.bvals = old->bt.bvals;
  a.bvals2 = fresh->bt.bvals;
  launch_prolong_flux_bc(k, a, stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(stream));
  return EQLB_OK;
}
} // namespace
} // namespace eqlb

extern "C" {

int eqlb_refine_facet_types(eqlb_refine_t* plan, eqlb_mesh_t* refined, int32_t nrhs, const int8_t* facet_type,
                            int8_t* facet_type2, int32_t memspace, void* stream_)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_refine_facet_types";
  if (!plan || !refined || !facet_type || !facet_type2)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  if (nrhs < 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: nrhs = %d (at least 1)", who, (int)nrhs);
  EQLB_TRY(check_memspace(who, memspace));
  CarryArgs a;
  EQLB_TRY(carry_args(who, plan, refined, a));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool host = memspace == EQLB_MEM_HOST;
  HostCall s; // (a device-memory call stages nothing: no allocation, no copy and no wait)
  const auto d_ft = s.in(host ? facet_type : nullptr, (size_t)nrhs * a.nfacets);
  const auto d_ft2 = s.out(host ? facet_type2 : nullptr, (size_t)nrhs * a.nfacets2);
  if (host)
    HIP_TRY(s.upload(stream));
  a.nrhs = nrhs;
  a.ft = host ? d_ft.get() : facet_type;
  a.ft2_out = host ? d_ft2.get() : facet_type2;
  if (a.nfacets2 > 0)
    hipLaunchKernelGGL(k_carry_facet_types, dim3(grid_of(a.nfacets2, CB_THREADS)), dim3(CB_THREADS), 0, stream, a);
  s.note(hipGetLastError());
  HIP_TRY(s.finish(stream));
  return EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_refine_child_facets(eqlb_refine_t* plan, eqlb_mesh_t* refined, int32_t nlist, const int32_t* facets,
                             int32_t* children, int32_t memspace, void* stream_)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_refine_child_facets";
  if (!plan || !refined)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  if (nlist < 0 || (nlist > 0 && (!facets || !children)))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: invalid list (nlist = %d)", who, (int)nlist);
  EQLB_TRY(check_memspace(who, memspace));
  CarryArgs a;
  EQLB_TRY(carry_args(who, plan, refined, a));
  const bool host = memspace == EQLB_MEM_HOST;
  if (host)
    for (int32_t i = 0; i < nlist; ++i)
      if (facets[i] < 0 || facets[i] >= a.nfacets)
        return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: facets[%d] = %d is no facet of the mesh", who, (int)i,
                    (int)facets[i]);
  if (nlist == 0)
    return EQLB_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  HostCall s;
  const auto d_list = s.in(host ? facets : nullptr, (size_t)nlist);
  const auto d_ch = s.out(host ? children : nullptr, 2 * (size_t)nlist);
  if (host)
    HIP_TRY(s.upload(stream));
  a.nlist = nlist;
  a.list = host ? d_list.get() : facets;
  a.children = host ? d_ch.get() : children;
  hipLaunchKernelGGL(k_child_facets, dim3(grid_of(nlist, CB_THREADS)), dim3(CB_THREADS), 0, stream, a);
  s.note(hipGetLastError());
  HIP_TRY(s.finish(stream));
  return EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_get_flux_bc_prolong_table(int32_t k, double* out, int32_t capacity)
{
  using namespace eqlb;
  if (k < 1 || k > 4 || !out)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_get_flux_bc_prolong_table: k = %d outside 1 ... 4, or null output",
                (int)k);
  const int n = 6 * k * k;
  if (capacity < n)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_get_flux_bc_prolong_table: capacity too small");
  const double* t = flux_bc_table(k);
  for (int i = 0; i < n; ++i)
    out[i] = t[i];
  return n;
}

int eqlb_refine_prolong_flux_bc(eqlb_refine_t* plan, eqlb_mesh_t* refined, int32_t k, int32_t nrhs,
                                const double* boundary_values, int32_t nlist, const int32_t* facets2, double* dofs,
                                int32_t memspace, void* stream_)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_refine_prolong_flux_bc";
  if (!plan || !refined || !boundary_values)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  if (k < 1 || k > 4)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: flux degree k = %d outside 1 ... 4", who, (int)k);
  if (nrhs < 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: nrhs = %d (at least 1)", who, (int)nrhs);
  if (nlist < 0 || (nlist > 0 && (!facets2 || !dofs)))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: invalid list (nlist = %d)", who, (int)nlist);
  EQLB_TRY(check_memspace(who, memspace));
  CarryArgs a;
  EQLB_TRY(carry_args(who, plan, refined, a));
  if (nlist == 0)
    return EQLB_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  a.nrhs = nrhs;
  a.nlist = nlist;
  if (memspace == EQLB_MEM_DEVICE)
  {
    a.list = facets2;
    a.bvals = boundary_values;
    a.dofs = dofs;
    launch_prolong_flux_bc(k, a, stream);
    HIP_TRY(hipGetLastError());
    return EQLB_OK;
  }
  // host memory: a pass that only checks the list, then the pass that writes - a refused list writes nothing
  const DeviceMesh& r = refined->m;
  const int32_t bad_init = INT32_MAX;
  int32_t bad = INT32_MAX;
  HostCall s;
  const auto d_list = s.in(facets2, (size_t)nlist);
  const auto d_bv = s.in(boundary_values, (size_t)nrhs * a.ncells * k * (k + 2));
  const auto d_bad = s.in(&bad_init, 1);
  const auto d_dofs = s.scratch<double>((size_t)nrhs * nlist * k);
  s.out_prefix(&bad, d_bad, 1);
  HIP_TRY(s.upload(stream));
  a.list = d_list;
  a.bvals = d_bv;
  a.dofs = d_dofs;
  a.first_bad = d_bad;
  launch_prolong_flux_bc(k, a, stream);
  s.note(hipGetLastError());
  HIP_TRY(s.finish(stream));
  if (bad != INT32_MAX)
  {
    const int32_t i = bad, f = (i >= 0 && i < nlist) ? facets2[i] : -1;
    if (f < 0 || f >= r.nfacets)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: facets2[%d] = %d is no facet of the refined mesh", who, (int)i, (int)f);
    if (refined->host.facet_cells_off[(size_t)f + 1] - refined->host.facet_cells_off[f] != 1)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: facets2[%d] = %d lies between two cells", who, (int)i, (int)f);
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: facets2[%d] = %d has no parent facet", who, (int)i, (int)f);
  }
  a.first_bad = nullptr;
  s.out_prefix(dofs, d_dofs, (size_t)nrhs * nlist * k);
  launch_prolong_flux_bc(k, a, stream);
  s.note(hipGetLastError());
  HIP_TRY(s.finish(stream));
  return EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_se_carry_boundary(const eqlb_se_t* old, eqlb_refine_t* plan, eqlb_se_t* fresh, const uint8_t* node_mask2,
                           void* stream)
try
{
  return eqlb::carry_boundary("eqlb_se_carry_boundary", "se", old, plan, fresh, nullptr, node_mask2, stream);
}
EQLB_CATCH_ALL

int eqlb_ev_carry_boundary(const eqlb_ev_t* old, eqlb_refine_t* plan, eqlb_ev_t* fresh, const uint8_t* node_mask2,
                           void* stream)
try
{
  if (!old || !plan || !fresh)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_ev_carry_boundary: null argument");
  return eqlb::carry_boundary("eqlb_ev_carry_boundary", "ev", old->se.get(), plan, fresh->se.get(), fresh, node_mask2, stream);
}
EQLB_CATCH_ALL

} // extern "C"
