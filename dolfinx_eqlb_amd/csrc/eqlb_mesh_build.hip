// Mesh connectivity ON THE DEVICE from coordinates and cells (eqlb_mesh_create_from_cells), and the small entries
// that read a mesh handle back: counts, export of the tables, boundary facets, facet ids of node pairs.
//
// The reference receives a finished topology from DOLFINx (FluxEquilibrator.initialise_mesh_info,
// python/dolfinx_eqlb/eqlb/FluxEquilibrator.py:52-67: connectivities 0<->1, 0<->2, 1<->2 and the facet
// permutations); every step of its adaptive demos builds it anew after mesh.refine.  Here the numbering is the one of
// dolfinx_eqlb_amd.mesh.create_mesh, bit for bit:
//   facets       unique edges in ascending order of the 64-bit key min(a, b) * nnodes + max(a, b), low node first
//   cell_facets  local facet f opposite local vertex f (vertex pairs [1,2], [0,2], [0,1])
//   facet_perm   first vertex of that pair > second
//   CSR tables   ascending entries, empty rows for nodes that no cell uses
//
// The build, everything on the caller's stream:
//   A  k_edge_keys      3 ncells keys with the value 3 cell + f, facet_perm; validates the cell (index range, repeated
//                       node) - the keys are formed from the indices themselves, nothing is dereferenced with them
//      radix_sort_pairs one stable sort of (key, value)
//      k_facet_heads    head flag per sorted position; a key that equals the one two positions before it is an edge
//                       of more than two cells
//      inclusive_scan   facet id + 1 per position; the last entry is nfacets
//      -> the error words and nfacets are read back; a refusal ends the call here, before x or any per-node table
//         is touched
//      k_facet_tables   the sort is stable, so the run of a key is ascending in the cell: facet_cells is a gather, the
//                       head positions are its offsets; cell_facets[value] = id, facet_nodes from the head keys
//   B  node -> cell and node -> facet: (node, cell) / (node, facet) pairs in ascending order of the second entry, one
//      stable sort by the node each; the offsets are filled from the boundaries of the sorted runs (k_csr_offsets:
//      the first position of every run writes the rows between the previous node and its own - histogram and scan in
//      one pass, without atomics)
//      k_node_counts    cells, facets and one-cell facets per node; rocprim::reduce gives the largest patch
//   C  cell geometry, download of the host copies the planner reads, one synchronisation
// Integer work only; the only atomics are atomicMin on the error words; two runs give the same bits.
//
// Device memory, N = 3 ncells, F = nfacets: the handle keeps what eqlb_mesh_create keeps plus node_cells.  On top of
// that the build holds one pool of 28 N bytes (two 8 N key buffers, two 4 N value buffers, 4 N facet ids: 84 bytes
// per cell) and the work space of rocPRIM (a few MB at 1M cells), both freed before the call returns; phase B
// reuses the pool (2 F <= 2 N entries of 4 bytes fit the 8 N buffers).
#include "eqlb_mesh_handle.h" // (eqlb_host_util.h)
#include "eqlb_topology_check.h"

#include <cstring> // (rocprim's texture iterator calls memset)
#include <rocprim/rocprim.hpp>

#include <climits>
#include <memory>

namespace eqlb
{
namespace
{
// error words of the build and the two numbers the host waits for
struct BuildWords
{
  int32_t range_cell;            // lowest cell with a node index outside [0, nnodes), INT32_MAX: none
  int32_t repeat_cell;           // lowest cell with a repeated node
  unsigned long long shared_key; // lowest key of an edge with more than two cells, ~0: none
  int32_t nfacets;
  int32_t ncells_max;
};

__global__ void __launch_bounds__(256)
k_edge_keys(int32_t ncells, int32_t nnodes, const int32_t* __restrict__ cell_nodes, unsigned long long* __restrict__ keys,
            int32_t* __restrict__ vals, uint8_t* __restrict__ facet_perm, BuildWords* w)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncells)
    return;
  const int32_t a[3] = {cell_nodes[3 * c], cell_nodes[3 * c + 1], cell_nodes[3 * c + 2]};
  bool in_range = true;
  for (int i = 0; i < 3; ++i)
    in_range = in_range && a[i] >= 0 && a[i] < nnodes;
  if (!in_range)
    atomicMin(&w->range_cell, (int32_t)c);
  else if (a[0] == a[1] || a[0] == a[2] || a[1] == a[2])
    atomicMin(&w->repeat_cell, (int32_t)c);
  for (int f = 0; f < 3; ++f)
  {
    const int32_t p = a[f == 0 ? 1 : 0], q = a[f == 2 ? 1 : 2];
    const long long lo = p < q ? p : q, hi = p < q ? q : p;
    keys[3 * c + f] = (unsigned long long)(lo * nnodes + hi); // (of a refused cell: some number, never an index)
    vals[3 * c + f] = (int32_t)(3 * c + f);
    facet_perm[3 * c + f] = p > q;
  }
}

__global__ void __launch_bounds__(256)
k_facet_heads(int64_t n, const unsigned long long* __restrict__ keys, int32_t* __restrict__ heads, BuildWords* w)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const unsigned long long k = keys[i];
  heads[i] = (i == 0 || keys[i - 1] != k);
  if (i >= 2 && keys[i - 2] == k)
    atomicMin(&w->shared_key, k);
}

__global__ void __launch_bounds__(256)
k_facet_tables(int64_t n, int32_t nnodes, int32_t nfacets, const unsigned long long* __restrict__ keys,
               const int32_t* __restrict__ vals, const int32_t* __restrict__ fid, int32_t* __restrict__ cell_facets,
               int32_t* __restrict__ facet_cells, int32_t* __restrict__ facet_cells_off, int32_t* __restrict__ facet_nodes)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const int32_t f = fid[i] - 1, v = vals[i]; // 0 <= f < nfacets (scan of the head flags), 0 <= v < n (a permutation)
  cell_facets[v] = f;
  facet_cells[i] = v / 3;
  const unsigned long long k = keys[i];
  if (i == 0 || keys[i - 1] != k)
  {
    facet_cells_off[f] = (int32_t)i;
    const unsigned long long lo = k / (unsigned long long)nnodes;
    facet_nodes[2 * (int64_t)f] = (int32_t)lo;
    facet_nodes[2 * (int64_t)f + 1] = (int32_t)(k - lo * (unsigned long long)nnodes);
  }
  if (i == n - 1)
    facet_cells_off[nfacets] = (int32_t)n;
}

// (row, col) pairs of a table with `stride` rows per entry: keys = the rows, vals = entry index
__global__ void __launch_bounds__(256)
k_node_pairs(int64_t n, int32_t stride, const int32_t* __restrict__ rows, uint32_t* __restrict__ keys,
             int32_t* __restrict__ vals)
{
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n)
    return;
  keys[j] = (uint32_t)rows[j];
  vals[j] = (int32_t)(j / stride);
}

// CSR offsets [nrows + 1] of n sorted row numbers: position i is the start of the rows in (keys[i-1], keys[i]]
__global__ void __launch_bounds__(256)
k_csr_offsets(int64_t n, int32_t nrows, const uint32_t* __restrict__ keys, int32_t* __restrict__ off)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n)
    return;
  const int64_t lo = (i == 0) ? 0 : (int64_t)keys[i - 1] + 1;
  const int64_t hi = (i == n) ? nrows : (int64_t)keys[i]; // keys < nrows: validated node indices
  for (int64_t r = lo; r <= hi; ++r)
    off[r] = (int32_t)i;
}

__global__ void __launch_bounds__(256)
k_node_counts(int32_t nnodes, const int32_t* __restrict__ node_cells_off, const int32_t* __restrict__ node_facets_off,
              const int32_t* __restrict__ node_facets, const int32_t* __restrict__ facet_cells_off,
              int32_t* __restrict__ ncells, int32_t* __restrict__ nfcts, int32_t* __restrict__ nbnd)
{
  const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnodes)
    return;
  const int32_t nf = node_facets_off[i + 1] - node_facets_off[i];
  ncells[i] = node_cells_off[i + 1] - node_cells_off[i];
  nfcts[i] = nf;
  nbnd[i] = node_boundary_facets(node_facets + node_facets_off[i], nf, facet_cells_off);
}

__global__ void __launch_bounds__(256)
k_boundary_flags(int32_t nfacets, const int32_t* __restrict__ facet_cells_off, int32_t* __restrict__ flag)
{
  const int32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f < nfacets)
    flag[f] = (facet_cells_off[f + 1] - facet_cells_off[f] == 1);
}

// pos: inclusive scan of the flags; facet f is listed at pos[f] - 1 if pos steps there
__global__ void __launch_bounds__(256)
k_boundary_scatter(int32_t nfacets, const int32_t* __restrict__ pos, int32_t* __restrict__ out)
{
  const int32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nfacets)
    return;
  const int32_t p = pos[f];
  if (p != (f ? pos[f - 1] : 0))
    out[p - 1] = f;
}

__global__ void __launch_bounds__(256)
k_find_facets(int32_t npairs, int32_t nnodes, const int32_t* __restrict__ pairs, const int32_t* __restrict__ node_facets_off,
              const int32_t* __restrict__ node_facets, const int32_t* __restrict__ facet_nodes, int32_t* __restrict__ out)
{
  const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npairs)
    return;
  const int32_t a = pairs[2 * (int64_t)i], b = pairs[2 * (int64_t)i + 1];
  int32_t found = -1;
  if (a >= 0 && a < nnodes && b >= 0 && b < nnodes)
    for (int32_t q = node_facets_off[a]; q < node_facets_off[a + 1] && found < 0; ++q)
    {
      const int32_t f = node_facets[q];
      const int32_t n0 = facet_nodes[2 * (int64_t)f], n1 = facet_nodes[2 * (int64_t)f + 1];
      if ((n0 == a && n1 == b) || (n0 == b && n1 == a))
        found = f;
    }
  out[i] = found;
}

inline unsigned bits_of(unsigned long long v) // bits needed for the values 0 ... v
{
  unsigned b = 1;
  while (b < 64 && (v >> b))
    ++b;
  return b;
}

const char* const WHO = "eqlb_mesh_create_from_cells";

int build_mesh(int32_t nnodes, int32_t ncells, const double* x, const int32_t* cell_nodes, int32_t memspace,
               hipStream_t stream, eqlb_mesh_t** mesh)
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
  const int64_t n3 = 3 * (int64_t)ncells;
  const hipMemcpyKind in_kind = memspace == EQLB_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  std::unique_ptr<eqlb_mesh> owner(new eqlb_mesh());
  eqlb_mesh& o = *owner; // the buffers; the view d learns of them when the last one is allocated
  DeviceMesh& d = o.m;
  HostMesh& hm = o.host;
  d.nnodes = nnodes;
  d.ncells = ncells;

  // ---- phase A: facets ------------------------------------------------------------------------------------------
  EQLB_TRY(o.cell_nodes.alloc((size_t)n3));
  EQLB_TRY(o.cell_facets.alloc((size_t)n3));
  EQLB_TRY(o.facet_perm.alloc((size_t)n3));
  HIP_TRY(hipMemcpyAsync(o.cell_nodes, cell_nodes, sizeof(int32_t) * (size_t)n3, in_kind, stream));

  DevCarve pool;
  const auto p_keys_in = pool.piece<unsigned long long>((size_t)n3), p_keys_out = pool.piece<unsigned long long>((size_t)n3);
  const auto p_vals_in = pool.piece<int32_t>((size_t)n3), p_vals_out = pool.piece<int32_t>((size_t)n3),
             p_fid = pool.piece<int32_t>((size_t)n3);
  DevBuf<char> tmp;
  DevBuf<BuildWords> words;
  if (pool.alloc() != hipSuccess)
    return fail(EQLB_ERR_DEVICE, "%s: device allocation failed", WHO);
  EQLB_TRY(words.alloc(1));
  unsigned long long *keys_in = p_keys_in, *keys_out = p_keys_out;
  int32_t *vals_in = p_vals_in, *vals_out = p_vals_out, *fid = p_fid;

  const unsigned key_bits = bits_of((unsigned long long)nnodes * (unsigned long long)nnodes - 1ull);
  size_t t_sort = 0, t_scan = 0;
  HIP_TRY(rocprim::radix_sort_pairs(nullptr, t_sort, keys_in, keys_out, vals_in, vals_out, (size_t)n3, 0u, key_bits,
                                    stream));
  HIP_TRY(rocprim::inclusive_scan(nullptr, t_scan, fid, fid, (size_t)n3, rocprim::plus<int32_t>(), stream));
  size_t tmp_bytes = std::max(t_sort, t_scan);
  EQLB_TRY(tmp.alloc(tmp_bytes));
  lap("from_cells: alloc + upload");

  HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(words.get()), INT32_MAX, 2, stream));
  HIP_TRY(hipMemsetAsync(&words.get()->shared_key, 0xff, sizeof(unsigned long long), stream));
  HIP_TRY(hipMemsetAsync(&words.get()->nfacets, 0, 2 * sizeof(int32_t), stream));
  hipLaunchKernelGGL(k_edge_keys, dim3(grid_of(ncells)), dim3(256), 0, stream, ncells, nnodes, o.cell_nodes, keys_in,
                     vals_in, o.facet_perm, words.get());
  {
    size_t tb = tmp_bytes;
    HIP_TRY(rocprim::radix_sort_pairs(tmp.get(), tb, keys_in, keys_out, vals_in, vals_out, (size_t)n3, 0u, key_bits,
                                      stream));
  }
  hipLaunchKernelGGL(k_facet_heads, dim3(grid_of(n3)), dim3(256), 0, stream, n3, keys_out, fid, words.get());
  {
    size_t tb = tmp_bytes;
    HIP_TRY(rocprim::inclusive_scan(tmp.get(), tb, fid, fid, (size_t)n3, rocprim::plus<int32_t>(), stream));
  }
  HIP_TRY(hipMemcpyAsync(&words.get()->nfacets, fid + (n3 - 1), sizeof(int32_t), hipMemcpyDeviceToDevice, stream));
  BuildWords w;
  HIP_TRY(hipMemcpyAsync(&w, words.get(), sizeof(w), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipGetLastError());
  lap("from_cells: facets (sort, scan)");
  if (w.range_cell != INT32_MAX)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: cell %d has a node index outside [0, %d)", WHO, w.range_cell, nnodes);
  if (w.repeat_cell != INT32_MAX)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: cell %d repeats a node", WHO, w.repeat_cell);
  if (w.shared_key != ~0ull)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: the edge between the nodes %lld and %lld is shared by more than two cells",
                WHO, (long long)(w.shared_key / (unsigned long long)nnodes),
                (long long)(w.shared_key % (unsigned long long)nnodes));
  const int32_t nfacets = w.nfacets;
  if (nfacets < 1 || (int64_t)nfacets > n3)
    return fail(EQLB_ERR_DEVICE, "%s: facet count %d out of range", WHO, nfacets);
  d.nfacets = nfacets;
  const int64_t n2 = 2 * (int64_t)nfacets;

  EQLB_TRY(o.facet_nodes.alloc((size_t)n2));
  EQLB_TRY(o.facet_cells_off.alloc((size_t)nfacets + 1));
  EQLB_TRY(o.facet_cells.alloc((size_t)n3));
  hipLaunchKernelGGL(k_facet_tables, dim3(grid_of(n3)), dim3(256), 0, stream, n3, nnodes, nfacets, keys_out, vals_out,
                     fid, o.cell_facets, o.facet_cells, o.facet_cells_off, o.facet_nodes);

  // ---- phase B: the per-node tables (every node index is known to be valid from here on) ----------------------
  EQLB_TRY(o.x.alloc((size_t)nnodes * 3));
  HIP_TRY(hipMemcpyAsync(o.x, x, sizeof(double) * (size_t)nnodes * 3, in_kind, stream));
  EQLB_TRY(o.node_cells_off.alloc((size_t)nnodes + 1));
  EQLB_TRY(o.node_cells.alloc((size_t)n3));
  EQLB_TRY(o.node_facets_off.alloc((size_t)nnodes + 1));
  EQLB_TRY(o.node_facets.alloc((size_t)n2));
  EQLB_TRY(o.cellJ.alloc((size_t)ncells * 4));
  o.publish();
  // the pool again: three buffers of max(n3, n2) <= 2 n3 entries of 4 bytes (the third runs over the two value
  // pieces, which follow each other)
  uint32_t* nk_in = reinterpret_cast<uint32_t*>(keys_in);
  uint32_t* nk_out = reinterpret_cast<uint32_t*>(keys_out);
  int32_t* nv_in = vals_in;
  const unsigned node_bits = bits_of((unsigned long long)nnodes - 1ull);
  DevBuf<char> tmp_b;
  DevBuf<int32_t> cnt; // [3][nnodes] cells, facets, one-cell facets per node
  EQLB_TRY(cnt.alloc(3 * (size_t)nnodes));
  size_t tb_c = 0, tb_f = 0, tb_r = 0;
  HIP_TRY(rocprim::radix_sort_pairs(nullptr, tb_c, nk_in, nk_out, nv_in, o.node_cells.get(), (size_t)n3, 0u, node_bits,
                                    stream));
  HIP_TRY(rocprim::radix_sort_pairs(nullptr, tb_f, nk_in, nk_out, nv_in, o.node_facets.get(), (size_t)n2, 0u, node_bits,
                                    stream));
  HIP_TRY(rocprim::reduce(nullptr, tb_r, cnt.get(), &words.get()->ncells_max, (int32_t)0, (size_t)nnodes,
                          rocprim::maximum<int32_t>(), stream));
  const size_t tmp_b_bytes = std::max(tb_c, std::max(tb_f, tb_r));
  EQLB_TRY(tmp_b.alloc(tmp_b_bytes));

  // the facet tables have been written: keys_out / vals_out / fid are free (same stream)
  hipLaunchKernelGGL(k_node_pairs, dim3(grid_of(n3)), dim3(256), 0, stream, n3, 3, o.cell_nodes, nk_in, nv_in);
  {
    size_t tb = tmp_b_bytes;
    HIP_TRY(rocprim::radix_sort_pairs(tmp_b.get(), tb, nk_in, nk_out, nv_in, o.node_cells.get(), (size_t)n3, 0u, node_bits,
                                      stream));
  }
  hipLaunchKernelGGL(k_csr_offsets, dim3(grid_of(n3 + 1)), dim3(256), 0, stream, n3, nnodes, nk_out, o.node_cells_off);
  hipLaunchKernelGGL(k_node_pairs, dim3(grid_of(n2)), dim3(256), 0, stream, n2, 2, o.facet_nodes, nk_in, nv_in);
  {
    size_t tb = tmp_b_bytes;
    HIP_TRY(rocprim::radix_sort_pairs(tmp_b.get(), tb, nk_in, nk_out, nv_in, o.node_facets.get(), (size_t)n2, 0u, node_bits,
                                      stream));
  }
  hipLaunchKernelGGL(k_csr_offsets, dim3(grid_of(n2 + 1)), dim3(256), 0, stream, n2, nnodes, nk_out, o.node_facets_off);
  int32_t *c_nc = cnt.get(), *c_nf = cnt.get() + nnodes, *c_nb = cnt.get() + 2 * (size_t)nnodes;
  hipLaunchKernelGGL(k_node_counts, dim3(grid_of(nnodes)), dim3(256), 0, stream, nnodes, o.node_cells_off,
                     o.node_facets_off, o.node_facets, o.facet_cells_off, c_nc, c_nf, c_nb);
  {
    size_t tb = tmp_b_bytes;
    HIP_TRY(rocprim::reduce(tmp_b.get(), tb, c_nc, &words.get()->ncells_max, (int32_t)0, (size_t)nnodes,
                            rocprim::maximum<int32_t>(), stream));
  }
  launch_cell_geometry(ncells, o.x, o.cell_nodes, o.cellJ, stream);
  lap("from_cells: node tables (2 sorts)");

  // ---- phase C: the host copies ---------------------------------------------------------------------------------
  auto down = [&](std::vector<int32_t>& h, const int32_t* src, size_t n) {
    h.resize(n);
    return hipMemcpyAsync(h.data(), src, sizeof(int32_t) * n, hipMemcpyDeviceToHost, stream);
  };
  HIP_TRY(down(hm.node_ncells, c_nc, (size_t)nnodes));
  HIP_TRY(down(hm.node_nfcts, c_nf, (size_t)nnodes));
  HIP_TRY(down(hm.node_nbnd, c_nb, (size_t)nnodes));
  HIP_TRY(down(hm.facet_cells_off, o.facet_cells_off, (size_t)nfacets + 1));
  HIP_TRY(down(hm.facet_nodes, o.facet_nodes, (size_t)n2));
  HIP_TRY(down(hm.node_facets_off, o.node_facets_off, (size_t)nnodes + 1));
  HIP_TRY(down(hm.node_facets, o.node_facets, (size_t)n2));
  HIP_TRY(down(hm.node_cells_off, o.node_cells_off, (size_t)nnodes + 1));
  HIP_TRY(down(hm.node_cells, o.node_cells, (size_t)n3));
  HIP_TRY(hipMemcpyAsync(&w, words.get(), sizeof(w), hipMemcpyDeviceToHost, stream));
  if (memspace == EQLB_MEM_HOST)
  {
    hm.x.assign(x, x + (size_t)nnodes * 3);
    hm.cell_nodes.assign(cell_nodes, cell_nodes + (size_t)n3);
  }
  else
  {
    hm.x.resize((size_t)nnodes * 3);
    HIP_TRY(hipMemcpyAsync(hm.x.data(), o.x, sizeof(double) * hm.x.size(), hipMemcpyDeviceToHost, stream));
    HIP_TRY(down(hm.cell_nodes, o.cell_nodes, (size_t)n3));
  }
  device_tiling_prepare(); // as eqlb_mesh_create: the code object of the tile builder is loaded here
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipGetLastError());
  d.ncells_max = w.ncells_max;
  lap("from_cells: download");
  *mesh = owner.release();
  return EQLB_OK;
}

} // namespace
} // namespace eqlb

extern "C" {

int eqlb_mesh_create_from_cells(int32_t nnodes, int32_t ncells, const double* x, const int32_t* cell_nodes,
                                int32_t memspace, void* stream, eqlb_mesh_t** mesh)
try
{
  if (!mesh || nnodes <= 0 || ncells <= 0 || !x || !cell_nodes)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null or empty input", eqlb::WHO);
  EQLB_TRY(eqlb::check_memspace(eqlb::WHO, memspace));
  if (3 * (int64_t)ncells > INT32_MAX)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: 3 * ncells = %lld does not fit 32 bits", eqlb::WHO,
                (long long)(3 * (int64_t)ncells));
  if (eqlb_device_count() < 1)
    return fail(EQLB_ERR_DEVICE, "%s: no HIP device available", eqlb::WHO);
  return eqlb::build_mesh(nnodes, ncells, x, cell_nodes, memspace, reinterpret_cast<hipStream_t>(stream), mesh);
}
EQLB_CATCH_ALL

int eqlb_mesh_counts(const eqlb_mesh_t* mesh, int32_t* nnodes, int32_t* ncells, int32_t* nfacets)
{
  if (!mesh)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_mesh_counts: null mesh");
  if (nnodes)
    *nnodes = mesh->m.nnodes;
  if (ncells)
    *ncells = mesh->m.ncells;
  if (nfacets)
    *nfacets = mesh->m.nfacets;
  return EQLB_OK;
}

int eqlb_mesh_export(eqlb_mesh_t* mesh, int32_t* cell_facets, int32_t* facet_nodes, int32_t* facet_cells_offsets,
                     int32_t* facet_cells, int32_t* node_cells_offsets, int32_t* node_cells,
                     int32_t* node_facets_offsets, int32_t* node_facets, uint8_t* facet_perm, int32_t memspace,
                     void* stream_)
{
  if (!mesh)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_mesh_export: null mesh");
  EQLB_TRY(eqlb::check_memspace("eqlb_mesh_export", memspace));
  const eqlb::DeviceMesh& m = mesh->m;
  const eqlb::HostMesh& hm = mesh->host;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  // a handle of eqlb_mesh_create uploads this table on first use
  const int32_t* d_node_cells = nullptr;
  if (node_cells && eqlb::mesh_node_cells(mesh, &d_node_cells))
    return fail(EQLB_ERR_DEVICE, "eqlb_mesh_export: device allocation failed");
  const hipMemcpyKind kind = memspace == EQLB_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  const size_t n3 = 3 * (size_t)m.ncells, nn = (size_t)m.nnodes, nf = (size_t)m.nfacets;
  struct
  {
    void* dst;
    const void* src;
    size_t bytes;
  } const jobs[] = {
      {cell_facets, m.cell_facets, 4 * n3},
      {facet_nodes, m.facet_nodes, 8 * nf},
      {facet_cells_offsets, m.facet_cells_off, 4 * (nf + 1)},
      {facet_cells, m.facet_cells, 4 * (size_t)hm.facet_cells_off[nf]},
      {node_cells_offsets, m.node_cells_off, 4 * (nn + 1)},
      {node_cells, d_node_cells, 4 * (size_t)hm.node_cells_off[nn]},
      {node_facets_offsets, m.node_facets_off, 4 * (nn + 1)},
      {node_facets, m.node_facets, 4 * (size_t)hm.node_facets_off[nn]},
      {facet_perm, m.facet_perm, n3},
  };
  for (const auto& j : jobs)
    if (j.dst && j.bytes)
      HIP_TRY(hipMemcpyAsync(j.dst, j.src, j.bytes, kind, stream));
  if (memspace == EQLB_MEM_HOST)
    HIP_TRY(hipStreamSynchronize(stream));
  return EQLB_OK;
}

int eqlb_mesh_boundary_facets(eqlb_mesh_t* mesh, int32_t* facets, int32_t capacity, int32_t* n, int32_t memspace,
                              void* stream_)
try
{
  if (!mesh || !n || capacity < 0 || (!facets && capacity > 0))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_mesh_boundary_facets: invalid argument");
  EQLB_TRY(eqlb::check_memspace("eqlb_mesh_boundary_facets", memspace));
  const eqlb::DeviceMesh& m = mesh->m;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const int32_t nf = m.nfacets;
  const bool host = memspace == EQLB_MEM_HOST;
  size_t tb = 0;
  HIP_TRY(rocprim::inclusive_scan(nullptr, tb, (int32_t*)nullptr, (int32_t*)nullptr, (size_t)nf,
                                  rocprim::plus<int32_t>(), stream));
  int32_t count = 0;
  eqlb::HostCall s;
  const auto pos = s.scratch<int32_t>((size_t)nf);
  const auto tmp = s.scratch<char>(tb);
  const auto staged = s.scratch<int32_t>(host ? (size_t)std::min(capacity, nf) : 0);
  s.out_prefix(&count, pos.at((size_t)nf - 1), 1);
  HIP_TRY(s.upload(stream));
  hipLaunchKernelGGL(eqlb::k_boundary_flags, dim3(eqlb::grid_of(nf)), dim3(256), 0, stream, nf, m.facet_cells_off,
                     pos.get());
  HIP_TRY(rocprim::inclusive_scan(tmp.get(), tb, pos.get(), pos.get(), (size_t)nf, rocprim::plus<int32_t>(), stream));
  HIP_TRY(s.finish(stream));
  *n = count;
  if (count > capacity)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_mesh_boundary_facets: capacity %d, the mesh has %d boundary facets",
                capacity, count);
  if (count == 0)
    return EQLB_OK;
  hipLaunchKernelGGL(eqlb::k_boundary_scatter, dim3(eqlb::grid_of(nf)), dim3(256), 0, stream, nf, pos.get(),
                     host ? staged.get() : facets);
  s.note(hipGetLastError());
  if (host)
    s.out_prefix(facets, staged, (size_t)count);
  HIP_TRY(s.finish(stream)); // (in either memory space: the scan buffer ends with this call)
  return EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_mesh_find_facets(eqlb_mesh_t* mesh, int32_t npairs, const int32_t* node_pairs, int32_t* facets,
                          int32_t memspace, void* stream_)
try
{
  if (!mesh || npairs < 0 || (npairs > 0 && (!node_pairs || !facets)))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_mesh_find_facets: invalid argument");
  EQLB_TRY(eqlb::check_memspace("eqlb_mesh_find_facets", memspace));
  if (npairs == 0)
    return EQLB_OK;
  const eqlb::DeviceMesh& m = mesh->m;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (memspace == EQLB_MEM_DEVICE)
  {
    hipLaunchKernelGGL(eqlb::k_find_facets, dim3(eqlb::grid_of(npairs)), dim3(256), 0, stream, npairs, m.nnodes,
                       node_pairs, m.node_facets_off, m.node_facets, m.facet_nodes, facets);
    HIP_TRY(hipGetLastError());
    return EQLB_OK;
  }
  eqlb::HostCall s;
  const auto d_pairs = s.in(node_pairs, 2 * (size_t)npairs);
  const auto d_out = s.out(facets, (size_t)npairs);
  HIP_TRY(s.upload(stream));
  hipLaunchKernelGGL(eqlb::k_find_facets, dim3(eqlb::grid_of(npairs)), dim3(256), 0, stream, npairs, m.nnodes,
                     d_pairs.get(), m.node_facets_off, m.node_facets, m.facet_nodes, d_out.get());
  s.note(hipGetLastError());
  HIP_TRY(s.finish(stream));
  return EQLB_OK;
}
EQLB_CATCH_ALL

} // extern "C"
