// Refinement of the marked cells ON THE DEVICE: longest-edge closure and bisection (eqlb_mesh_refine_plan and the
// eqlb_refine_* entries) - the last step of the reference's adaptive loop that stayed with the caller
// (demo/poisson_adaptive/demo_lshape.py, demo_discont-coeff.py, demo/elasticity_adaptive/demo_cook.py:
// mesh.compute_incident_entities(mesh, marked, 2, 1), mesh.refine(mesh, edges), then the mesh information again).  The
// rule is stated in include/eqlb.h and, as numpy, in dolfinx_eqlb_amd/mesh/refine.py; the device reproduces the numpy
// statement bit for bit.
//
// The plan, everything on the caller's stream, one thread per facet or per cell:
//   k_facet_len2      len2[f] = dx dx + dy dy, every operation rounded on its own (contraction switched off in that
//                     kernel: hipcc would fuse the sum into a multiply-add, also through __dmul_rn / __dadd_rn)
//   k_cell_longest    l(c), and succ(c) = the other cell of L(c), c itself on the boundary
//   k_seed            E0 from the marked list; the count and every id are checked before they address anything
//   k_active          A0 = cells with a facet in E0
//   k_double          ceil(log2(ncells)) passes of jump <- jump o jump (double-buffered) and act[jump[c]] <- 1 for
//                     active c.  Invariant: after pass i, act holds every cell within 2^(i+1) - 1 steps of A0, and only
//                     cells reachable from A0 - whichever of the racing stores (all of the value 1) a read observes
//   k_longest_flags   E = E0 and L(c) for c in A
//   k_child_counts    1 + facets in E per cell
//   exclusive_scan    (rocPRIM) new-node rank per facet, first child per cell; the totals are the last entries
//   k_bisected        the facets of E in ascending order (node_parent_facet)
// then ONE wait for the error words and the counts.  eqlb_refine_write is two kernels (midpoints, children) and a copy
// of the old coordinates; eqlb_refine_parent_facets one kernel over the facets of the refined handle.
// The number of launches depends on ncells alone.  The flags are bytes (cells) and words (facets, scanned as they
// are); the only atomics are atomicMin on the error word and one integer add per wave for the count of cut cells.
#include "eqlb_refine_device.h"
#include "eqlb_refine_plan.h"

#include <cstring> // (rocprim's texture iterator calls memset)
#include <rocprim/rocprim.hpp>

#include <climits>
#include <memory>

namespace eqlb
{
namespace
{
struct RefineWords
{
  int32_t bad_id;      // lowest marked id outside [0, ncells); valid if has_bad
  int32_t has_bad;
  int32_t count_state; // 0 fine, 1: *nmarked < 0, 2: *nmarked > capacity
  int32_t ncut;        // cells with a facet in E
  long long nmarked;   // the refused count
  int32_t nbis;        // facets in E
  uint32_t ncells2;
};

__global__ void __launch_bounds__(256)
k_facet_len2(int32_t nfacets, const double* __restrict__ x, const int32_t* __restrict__ facet_nodes,
             double* __restrict__ len2)
{
#pragma clang fp contract(off) // hipcc contracts by default, through the inlined __dmul_rn / __dadd_rn as well
  const int32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nfacets)
    return;
  const int64_t lo = facet_nodes[2 * (int64_t)f], hi = facet_nodes[2 * (int64_t)f + 1];
  const double dx = x[3 * hi] - x[3 * lo], dy = x[3 * hi + 1] - x[3 * lo + 1];
  const double dx2 = dx * dx, dy2 = dy * dy;
  len2[f] = dx2 + dy2;
}

__global__ void __launch_bounds__(256)
k_cell_longest(int32_t ncells, const int32_t* __restrict__ cell_facets, const double* __restrict__ len2,
               const int32_t* __restrict__ facet_cells_off, const int32_t* __restrict__ facet_cells,
               uint8_t* __restrict__ lloc, int32_t* __restrict__ succ)
{
  const int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncells)
    return;
  int32_t best = cell_facets[3 * (int64_t)c];
  double lbest = len2[best];
  int l = 0;
#pragma unroll
  for (int j = 1; j < 3; ++j)
  {
    const int32_t f = cell_facets[3 * (int64_t)c + j];
    const double lf = len2[f];
    if (lf > lbest || (lf == lbest && f < best))
    {
      best = f;
      lbest = lf;
      l = j;
    }
  }
  lloc[c] = (uint8_t)l;
  const int32_t o = facet_cells_off[best], n = facet_cells_off[best + 1] - o;
  int32_t s = c;
  if (n == 2)
  {
    const int32_t c0 = facet_cells[o], c1 = facet_cells[o + 1];
    s = (c0 == c) ? c1 : c0;
  }
  succ[c] = s;
}

__global__ void __launch_bounds__(256)
k_seed(int32_t ncells, const int32_t* __restrict__ marked, const long long* __restrict__ nmarked, long long capacity,
       const int32_t* __restrict__ cell_facets, int32_t* __restrict__ fE, RefineWords* w)
{
  const long long nm = *nmarked;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
  if (nm < 0 || nm > capacity)
  {
    if (t == 0)
    {
      w->count_state = nm < 0 ? 1 : 2;
      w->nmarked = nm;
    }
    return;
  }
  for (long long i = t; i < nm; i += stride)
  {
    const int32_t c = marked[i];
    if (c < 0 || c >= ncells)
    {
      atomicMin(&w->bad_id, c);
      w->has_bad = 1;
    }
    else
      for (int j = 0; j < 3; ++j)
        fE[cell_facets[3 * (int64_t)c + j]] = 1;
  }
}

__global__ void __launch_bounds__(256)
k_active(int32_t ncells, const int32_t* __restrict__ cell_facets, const int32_t* __restrict__ fE,
         uint8_t* __restrict__ act)
{
  const int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncells)
    return;
  const int32_t* cf = cell_facets + 3 * (int64_t)c;
  act[c] = (uint8_t)((fE[cf[0]] | fE[cf[1]] | fE[cf[2]]) != 0);
}

// act is read and written by different threads of the launch (stores of 1 only): no __restrict__
__global__ void __launch_bounds__(256)
k_double(int32_t ncells, const int32_t* __restrict__ jump_in, int32_t* __restrict__ jump_out, uint8_t* act)
{
  const int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncells)
    return;
  const int32_t j = jump_in[c];
  if (act[c])
    act[j] = 1;
  jump_out[c] = jump_in[j];
}

__global__ void __launch_bounds__(256)
k_longest_flags(int32_t ncells, const int32_t* __restrict__ cell_facets, const uint8_t* __restrict__ lloc,
                const uint8_t* __restrict__ act, int32_t* __restrict__ fE)
{
  const int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < ncells && act[c])
    fE[cell_facets[3 * (int64_t)c + lloc[c]]] = 1;
}

// threads 0 ... ncells: the entry behind the last cell is 0, so that the exclusive scan ends in the total
__global__ void __launch_bounds__(256)
k_child_counts(int32_t ncells, const int32_t* __restrict__ cell_facets, const int32_t* __restrict__ fE,
               uint32_t* __restrict__ nch, RefineWords* w)
{
  const int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  int32_t n = 0;
  if (c < ncells)
  {
    const int32_t* cf = cell_facets + 3 * (int64_t)c;
    n = fE[cf[0]] + fE[cf[1]] + fE[cf[2]];
    nch[c] = 1u + (uint32_t)n;
  }
  else if (c == ncells)
    nch[c] = 0u;
  const unsigned long long cut = __ballot(n > 0);
  if ((threadIdx.x & 63) == 0 && cut)
    atomicAdd(&w->ncut, (int32_t)__popcll(cut));
}

__global__ void __launch_bounds__(256)
k_bisected(int32_t nfacets, const int32_t* __restrict__ fE, const int32_t* __restrict__ frank,
           int32_t* __restrict__ bis_facet)
{
  const int32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f < nfacets && fE[f])
    bis_facet[frank[f]] = f; // 0 <= rank < number of flags <= nfacets
}

__global__ void __launch_bounds__(256)
k_write_nodes(int32_t nbis, int32_t nnodes, const int32_t* __restrict__ bis_facet,
              const int32_t* __restrict__ facet_nodes, const double* __restrict__ x, double* __restrict__ x2,
              int32_t* __restrict__ node_parent_facet)
{
  const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nbis)
    return;
  const int32_t f = bis_facet[r];
  if (node_parent_facet)
    node_parent_facet[r] = f;
  if (x2)
  {
    const int64_t lo = facet_nodes[2 * (int64_t)f], hi = facet_nodes[2 * (int64_t)f + 1];
    double* o = x2 + 3 * ((int64_t)nnodes + r);
    for (int i = 0; i < 3; ++i)
      o[i] = 0.5 * (x[3 * lo + i] + x[3 * hi + i]);
  }
}

__global__ void __launch_bounds__(256)
k_write_cells(int32_t ncells, int32_t nnodes, const int32_t* __restrict__ cell_nodes,
              const int32_t* __restrict__ cell_facets, const uint8_t* __restrict__ lloc,
              const int32_t* __restrict__ fE, const int32_t* __restrict__ frank, const uint32_t* __restrict__ coff,
              int32_t* __restrict__ cell_nodes2, int32_t* __restrict__ parent_cell)
{
  const int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncells)
    return;
  const int64_t first = coff[c];
  const int nchild = (int)(coff[c + 1] - coff[c]); // 1 ... 4
  if (parent_cell)
    for (int i = 0; i < nchild; ++i)
      parent_cell[first + i] = c;
  if (!cell_nodes2)
    return;
  const int32_t* v = cell_nodes + 3 * (int64_t)c;
  const int32_t* cf = cell_facets + 3 * (int64_t)c;
  int32_t* out = cell_nodes2 + 3 * first;
  auto put = [&](int i, int32_t n0, int32_t n1, int32_t n2) {
    out[3 * i] = n0;
    out[3 * i + 1] = n1;
    out[3 * i + 2] = n2;
  };
  if (nchild == 1)
  {
    put(0, v[0], v[1], v[2]);
    return;
  }
  const int l = lloc[c], l1 = (l + 1) % 3, l2 = (l + 2) % 3;
  const int32_t a = v[l], b = v[l1], cc = v[l2];
  const int32_t fm = cf[l], fq = cf[l1], fp = cf[l2];
  const int32_t m = nnodes + frank[fm]; // a cut cell has its longest facet in E
  int i = 0;
  if (fE[fp])
  {
    const int32_t p = nnodes + frank[fp];
    put(i++, a, p, m);
    put(i++, p, b, m);
  }
  else
    put(i++, a, b, m);
  if (fE[fq])
  {
    const int32_t q = nnodes + frank[fq];
    put(i++, a, m, q);
    put(i++, q, m, cc);
  }
  else
    put(i++, a, m, cc);
}

// one thread per facet of the refined handle; its node indices are < nnodes + nbis (checked by the caller)
__global__ void __launch_bounds__(256)
k_parent_facets(int32_t nfacets2, int32_t nnodes, const int32_t* __restrict__ facet_nodes2,
                const int32_t* __restrict__ bis_facet, const int32_t* __restrict__ facet_nodes,
                const int32_t* __restrict__ node_facets_off, const int32_t* __restrict__ node_facets,
                int32_t* __restrict__ parent_facet)
{
  const int32_t f2 = blockIdx.x * blockDim.x + threadIdx.x;
  if (f2 >= nfacets2)
    return;
  parent_facet[f2] = parent_facet_of(f2, nnodes, facet_nodes2, bis_facet, facet_nodes, node_facets_off, node_facets);
}

const char* const WHO = "eqlb_mesh_refine_plan";
} // namespace
} // namespace eqlb

namespace eqlb
{
namespace
{
int build_plan(const eqlb_mesh* mesh, const int32_t* marked, const int64_t* nmarked, int64_t capacity,
               int32_t memspace, hipStream_t stream, eqlb_refine_t** plan)
{
  SetupTimer tm;
  // EQLB_PROFILE_SETUP=1: the phases on stderr, each closed by a synchronisation of its own
  auto lap = [&](const char* what) {
    if (tm.on)
    {
      (void)hipStreamSynchronize(stream);
      tm.lap(what);
    }
  };
  const DeviceMesh& m = mesh->m;
  const int32_t nc = m.ncells, nf = m.nfacets;
  std::unique_ptr<eqlb_refine> p(new eqlb_refine());
  p->mesh = mesh;
  p->nnodes = m.nnodes;
  p->ncells = nc;
  p->nfacets = nf;

  DevBuf<int32_t> d_marked, succ, jump0, jump1;
  DevBuf<long long> d_nm;
  DevBuf<double> len2;
  DevBuf<uint8_t> act;
  DevBuf<uint32_t> nch;
  DevBuf<RefineWords> words;
  DevBuf<char> tmp;
  const int32_t* marked_d = marked;
  const long long* nm_d = reinterpret_cast<const long long*>(nmarked);
  long long seed_items = capacity;
  if (memspace == EQLB_MEM_HOST)
  {
    const long long nm = *nmarked; // checked by the caller
    EQLB_TRY(d_marked.alloc((size_t)nm));
    EQLB_TRY(d_nm.alloc(1));
    if (nm > 0)
      HIP_TRY(hipMemcpyAsync(d_marked.get(), marked, sizeof(int32_t) * (size_t)nm, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_nm.get(), nmarked, sizeof(long long), hipMemcpyHostToDevice, stream));
    marked_d = d_marked.get();
    nm_d = d_nm.get();
    seed_items = nm;
  }
  EQLB_TRY(p->fE.alloc((size_t)nf + 1));
  EQLB_TRY(p->frank.alloc((size_t)nf + 1));
  EQLB_TRY(p->bis_facet.alloc((size_t)nf));
  EQLB_TRY(p->coff.alloc((size_t)nc + 1));
  EQLB_TRY(p->lloc.alloc((size_t)nc));
  EQLB_TRY(len2.alloc((size_t)nf));
  EQLB_TRY(succ.alloc((size_t)nc));
  EQLB_TRY(jump0.alloc((size_t)nc));
  EQLB_TRY(jump1.alloc((size_t)nc));
  EQLB_TRY(act.alloc((size_t)nc));
  EQLB_TRY(nch.alloc((size_t)nc + 1));
  EQLB_TRY(words.alloc(1));
  size_t t_f = 0, t_c = 0;
  HIP_TRY(rocprim::exclusive_scan(nullptr, t_f, p->fE.get(), p->frank.get(), (int32_t)0, (size_t)nf + 1,
                                  rocprim::plus<int32_t>(), stream));
  HIP_TRY(rocprim::exclusive_scan(nullptr, t_c, nch.get(), p->coff.get(), (uint32_t)0, (size_t)nc + 1,
                                  rocprim::plus<uint32_t>(), stream));
  const size_t tmp_bytes = std::max(t_f, t_c);
  EQLB_TRY(tmp.alloc(tmp_bytes));
  lap("refine: alloc + upload");

  HIP_TRY(hipMemsetAsync(words.get(), 0, sizeof(RefineWords), stream));
  HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(words.get()), INT32_MAX, 1, stream));
  HIP_TRY(hipMemsetAsync(p->fE.get(), 0, sizeof(int32_t) * ((size_t)nf + 1), stream));
  hipLaunchKernelGGL(k_facet_len2, dim3(grid_of(nf)), dim3(256), 0, stream, nf, m.x, m.facet_nodes, len2.get());
  hipLaunchKernelGGL(k_cell_longest, dim3(grid_of(nc)), dim3(256), 0, stream, nc, m.cell_facets, len2.get(),
                     m.facet_cells_off, m.facet_cells, p->lloc.get(), succ.get());
  // the length of the list is known to the device only: a grid-stride loop over at most 1024 blocks
  const unsigned seed_grid = std::max(1u, std::min(1024u, grid_of(std::min<long long>(seed_items, INT32_MAX))));
  hipLaunchKernelGGL(k_seed, dim3(seed_grid), dim3(256), 0, stream, nc, marked_d, nm_d, (long long)capacity,
                     m.cell_facets, p->fE.get(), words.get());
  hipLaunchKernelGGL(k_active, dim3(grid_of(nc)), dim3(256), 0, stream, nc, m.cell_facets, p->fE.get(), act.get());
  {
    const int32_t* in = succ.get();
    int32_t* bufs[2] = {jump0.get(), jump1.get()};
    int pass = 0;
    for (int64_t reach = 1; reach < nc; reach *= 2, ++pass) // ceil(log2(ncells)) passes
    {
      hipLaunchKernelGGL(k_double, dim3(grid_of(nc)), dim3(256), 0, stream, nc, in, bufs[pass & 1], act.get());
      in = bufs[pass & 1];
    }
  }
  hipLaunchKernelGGL(k_longest_flags, dim3(grid_of(nc)), dim3(256), 0, stream, nc, m.cell_facets, p->lloc.get(),
                     act.get(), p->fE.get());
  lap("refine: closure");
  hipLaunchKernelGGL(k_child_counts, dim3(grid_of((int64_t)nc + 1)), dim3(256), 0, stream, nc, m.cell_facets,
                     p->fE.get(), nch.get(), words.get());
  {
    size_t tb = tmp_bytes;
    HIP_TRY(rocprim::exclusive_scan(tmp.get(), tb, p->fE.get(), p->frank.get(), (int32_t)0, (size_t)nf + 1,
                                    rocprim::plus<int32_t>(), stream));
    tb = tmp_bytes;
    HIP_TRY(rocprim::exclusive_scan(tmp.get(), tb, nch.get(), p->coff.get(), (uint32_t)0, (size_t)nc + 1,
                                    rocprim::plus<uint32_t>(), stream));
  }
  hipLaunchKernelGGL(k_bisected, dim3(grid_of(nf)), dim3(256), 0, stream, nf, p->fE.get(), p->frank.get(),
                     p->bis_facet.get());
  HIP_TRY(hipMemcpyAsync(&words.get()->nbis, p->frank.get() + nf, sizeof(int32_t), hipMemcpyDeviceToDevice, stream));
  HIP_TRY(hipMemcpyAsync(&words.get()->ncells2, p->coff.get() + nc, sizeof(uint32_t), hipMemcpyDeviceToDevice,
                         stream));
  RefineWords w;
  HIP_TRY(hipMemcpyAsync(&w, words.get(), sizeof(w), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipGetLastError());
  lap("refine: scans");
  if (w.count_state == 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT,
                "%s: nmarked = %lld (eqlb_mark_doerfler writes -1 for a negative or NaN indicator)", WHO, w.nmarked);
  if (w.count_state == 2)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: nmarked = %lld exceeds the capacity %lld", WHO, w.nmarked,
                (long long)capacity);
  if (w.has_bad)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: marked cell %d outside [0, %d)", WHO, w.bad_id, nc);
  if (3 * (int64_t)w.ncells2 > INT32_MAX)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: 3 * ncells2 = %lld does not fit 32 bits", WHO,
                (long long)(3 * (int64_t)w.ncells2));
  if (w.nbis < 0 || w.nbis > nf || w.ncells2 < (uint32_t)nc || (int64_t)m.nnodes + w.nbis > INT32_MAX)
    return fail(EQLB_ERR_DEVICE, "%s: counts out of range (%d bisected facets, %u cells)", WHO, w.nbis, w.ncells2);
  p->nbis = w.nbis;
  p->ncells2 = (int32_t)w.ncells2;
  p->ncut = w.ncut;
  *plan = p.release();
  return EQLB_OK;
}

// all pointers DEVICE (or nullptr); enqueues on stream
int enqueue_write(const eqlb_refine* p, double* x2, int32_t* cell_nodes2, int32_t* parent_cell,
                  int32_t* node_parent_facet, hipStream_t stream)
{
  const DeviceMesh& m = p->mesh->m;
  if (x2)
    HIP_TRY(hipMemcpyAsync(x2, m.x, sizeof(double) * 3 * (size_t)p->nnodes, hipMemcpyDeviceToDevice, stream));
  if (p->nbis > 0 && (x2 || node_parent_facet))
    hipLaunchKernelGGL(k_write_nodes, dim3(grid_of(p->nbis)), dim3(256), 0, stream, p->nbis, p->nnodes,
                       p->bis_facet.get(), m.facet_nodes, m.x, x2, node_parent_facet);
  if (cell_nodes2 || parent_cell)
    hipLaunchKernelGGL(k_write_cells, dim3(grid_of(p->ncells)), dim3(256), 0, stream, p->ncells, p->nnodes,
                       m.cell_nodes, m.cell_facets, p->lloc.get(), p->fE.get(), p->frank.get(), p->coff.get(),
                       cell_nodes2, parent_cell);
  HIP_TRY(hipGetLastError());
  return EQLB_OK;
}
} // namespace
} // namespace eqlb

extern "C" {

int eqlb_mesh_refine_plan(eqlb_mesh_t* mesh, const int32_t* marked, const int64_t* nmarked, int64_t capacity,
                          int32_t memspace, void* stream, eqlb_refine_t** plan)
try
{
  if (!mesh || !nmarked || !plan || capacity < 0 || (!marked && capacity > 0))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument or negative capacity", eqlb::WHO);
  EQLB_TRY(eqlb::check_memspace(eqlb::WHO, memspace));
  if (memspace == EQLB_MEM_HOST)
  {
    const long long nm = *nmarked;
    if (nm < 0)
      return fail(EQLB_ERR_INVALID_ARGUMENT,
                  "%s: nmarked = %lld (eqlb_mark_doerfler writes -1 for a negative or NaN indicator)", eqlb::WHO, nm);
    if (nm > capacity)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: nmarked = %lld exceeds the capacity %lld", eqlb::WHO, nm,
                  (long long)capacity);
  }
  return eqlb::build_plan(mesh, marked, nmarked, capacity, memspace, reinterpret_cast<hipStream_t>(stream), plan);
}
EQLB_CATCH_ALL

int eqlb_refine_counts(const eqlb_refine_t* plan, int32_t* nnodes2, int32_t* ncells2, int32_t* nbisected,
                       int32_t* ncells_cut)
{
  if (!plan)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_refine_counts: null plan");
  if (nnodes2)
    *nnodes2 = plan->nnodes + plan->nbis;
  if (ncells2)
    *ncells2 = plan->ncells2;
  if (nbisected)
    *nbisected = plan->nbis;
  if (ncells_cut)
    *ncells_cut = plan->ncut;
  return EQLB_OK;
}

int eqlb_refine_write(eqlb_refine_t* plan, double* x2, int32_t* cell_nodes2, int32_t* parent_cell,
                      int32_t* node_parent_facet, int32_t memspace, void* stream_)
try
{
  if (!plan)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_refine_write: null plan");
  EQLB_TRY(eqlb::check_memspace("eqlb_refine_write", memspace));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (memspace == EQLB_MEM_DEVICE)
    return eqlb::enqueue_write(plan, x2, cell_nodes2, parent_cell, node_parent_facet, stream);
  const size_t nx = 3 * ((size_t)plan->nnodes + (size_t)plan->nbis), n3 = 3 * (size_t)plan->ncells2,
               nc2 = (size_t)plan->ncells2, nb = (size_t)plan->nbis;
  eqlb::HostCall s;
  const auto d_x = s.out(x2, nx);
  const auto d_c = s.out(cell_nodes2, n3), d_pc = s.out(parent_cell, nc2), d_npf = s.out(node_parent_facet, nb);
  HIP_TRY(s.upload(stream));
  const int rc = eqlb::enqueue_write(plan, d_x, d_c, d_pc, d_npf, stream);
  HIP_TRY(s.finish(stream));
  return rc;
}
EQLB_CATCH_ALL

int eqlb_refine_create_mesh(eqlb_refine_t* plan, void* stream_, eqlb_mesh_t** refined)
try
{
  if (!plan || !refined)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_refine_create_mesh: null argument");
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const int32_t nnodes2 = plan->nnodes + plan->nbis;
  eqlb::DevBuf<double> d_x;
  eqlb::DevBuf<int32_t> d_c;
  EQLB_TRY(d_x.alloc(3 * (size_t)nnodes2));
  EQLB_TRY(d_c.alloc(3 * (size_t)plan->ncells2));
  EQLB_TRY(eqlb::enqueue_write(plan, d_x.get(), d_c.get(), nullptr, nullptr, stream));
  // (waits for the stream before it returns: the two arrays may be freed then)
  return eqlb_mesh_create_from_cells(nnodes2, plan->ncells2, d_x.get(), d_c.get(), EQLB_MEM_DEVICE, stream_, refined);
}
EQLB_CATCH_ALL

int eqlb_refine_parent_facets(eqlb_refine_t* plan, eqlb_mesh_t* refined, int32_t* parent_facet, int32_t memspace,
                              void* stream_)
try
{
  if (!plan || !refined || !parent_facet)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_refine_parent_facets: null argument");
  EQLB_TRY(eqlb::check_memspace("eqlb_refine_parent_facets", memspace));
  const eqlb::DeviceMesh &m = plan->mesh->m, &r = refined->m;
  if (r.nnodes != plan->nnodes + plan->nbis || r.ncells != plan->ncells2)
    return fail(EQLB_ERR_INVALID_ARGUMENT,
                "eqlb_refine_parent_facets: the handle has %d nodes and %d cells, the refined mesh %d and %d", r.nnodes,
                r.ncells, plan->nnodes + plan->nbis, plan->ncells2);
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const int32_t nf2 = r.nfacets;
  eqlb::HostCall s;
  const auto staged = s.out(memspace == EQLB_MEM_HOST ? parent_facet : nullptr, (size_t)nf2);
  if (memspace == EQLB_MEM_HOST)
    HIP_TRY(s.upload(stream));
  hipLaunchKernelGGL(eqlb::k_parent_facets, dim3(eqlb::grid_of(nf2)), dim3(256), 0, stream, nf2, plan->nnodes,
                     r.facet_nodes, plan->bis_facet.get(), m.facet_nodes, m.node_facets_off, m.node_facets,
                     memspace == EQLB_MEM_HOST ? staged.get() : parent_facet);
  s.note(hipGetLastError());
  HIP_TRY(s.finish(stream)); // (a device-memory call staged nothing: no copy and no wait)
  return EQLB_OK;
}
EQLB_CATCH_ALL

void eqlb_refine_destroy(eqlb_refine_t* plan) { delete plan; }

} // extern "C"
