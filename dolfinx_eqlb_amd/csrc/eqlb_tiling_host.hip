// Tiles of the tiled launch (EQLB_SCATTER_TILED) on the host: recursive coordinate bisection of the cell centroids
// (rcb_split) and the tiled patch SoA built from it (build_tiles, called by eqlb_se_set_boundary).  Host code only;
// the device bisection it tries first is eqlb_tiling_device.hip.
#include "eqlb_host_util.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <future>
#include <memory>
#include <mutex>
#include <thread>

namespace
{
// Recursive coordinate bisection of the cell centroids into chunks of exactly `tc` cells (the last
// one may be short): compact tiles keep the share of rim patches, which are solved by every tile
// they touch, small.
// (centroids relative to the bounding box of the mesh, in single precision: the bisection only compares them,
// ties go by the cell id, and a 12-byte item moves through the selection passes twice as fast as a 24-byte one)
struct TileItem
{
  float x, y;
  int32_t cell;
};

// Context of the bisection: cell -> nodes and a per-node stamp to count the nodes a cut separates
struct RcbCtx
{
  const int32_t* cell_nodes;
  std::vector<int64_t> stamp; // [nnodes] 2 * epoch + side of the last cell that touched the node
  std::vector<int64_t> cut;   // [nnodes] epoch in which the node was counted as cut
  int64_t epoch = 0;
};

static inline bool rcb_less(const TileItem& p, const TileItem& q, int axis)
{
  const float u = axis ? p.y : p.x, v = axis ? q.y : q.x;
  return u < v || (u == v && p.cell < q.cell);
}

// std::vector without value initialisation: the big scratch arrays of the tile builder are written completely by the
// worker threads - a zero fill by the calling thread would touch (page-fault) tens of MB serially first
template <typename T>
struct default_init_alloc : std::allocator<T>
{
  template <typename U>
  struct rebind
  {
    using other = default_init_alloc<U>;
  };
  template <typename U, typename... A>
  void construct(U* p, A&&... a)
  {
    if constexpr (sizeof...(A) == 0)
      ::new (static_cast<void*>(p)) U;
    else
      ::new (static_cast<void*>(p)) U(std::forward<A>(a)...);
  }
};
template <typename T>
using uvec = std::vector<T, default_init_alloc<T>>;

// Host worker threads of the set-up: capped (the tile builder keeps an O(nnodes) stamp per worker: 16 MB each at
// 4M nodes, on every rank of a node) and exception safe - an exception inside a std::thread would call
// std::terminate; the first one is kept and re-thrown by join() in the calling thread, where the C entry points
// turn it into an error code (EQLB_GUARD).
static int host_workers(int64_t wanted)
{
  const int64_t hw = std::max<int64_t>(1, std::min<int64_t>(std::thread::hardware_concurrency(), 32));
  return (int)std::max<int64_t>(1, std::min<int64_t>(hw, wanted));
}
struct Workers
{
  std::vector<std::thread> th;
  std::exception_ptr err;
  std::mutex mu;
  template <typename F>
  void spawn(F f)
  {
    th.emplace_back([this, f]() {
      try
      {
        f();
      }
      catch (...)
      {
        std::lock_guard<std::mutex> g(mu);
        if (!err)
          err = std::current_exception();
      }
    });
  }
  void join()
  {
    for (auto& x : th)
      x.join();
    th.clear();
    if (err)
    {
      std::exception_ptr e = err;
      err = nullptr;
      std::rethrow_exception(e);
    }
  }
  ~Workers()
  {
    for (auto& x : th)
      if (x.joinable())
        x.join();
  }
};

// The same partition as rcb_partition (the key (coordinate, cell id) is a total order, so the two halves are
// determined as SETS) on the host threads, for the few large segments at the top of the recursion where the
// subtrees do not yet occupy the cores: histogram of the coordinate -> bucket of the splitting element ->
// exact splitter inside that bucket -> counting partition through a scratch array.
static void rcb_partition_parallel(TileItem* a, int64_t n, int64_t nl, int axis, float lo, float hi,
                                   std::vector<TileItem>& tmp)
{
  const int nt = host_workers(n / (1 << 15));
  constexpr int NBK = 4096;
  const float scale = (hi > lo) ? (float)NBK / (hi - lo) : 0.0f;
  auto bucket = [&](const TileItem& t) {
    const int b = (int)(((axis ? t.y : t.x) - lo) * scale);
    return b < 0 ? 0 : (b >= NBK ? NBK - 1 : b);
  };
  auto run = [&](auto f) {
    Workers w;
    for (int t = 1; t < nt; ++t)
      w.spawn([f, t]() { f(t); });
    f(0);
    w.join();
  };
  std::vector<int64_t> hist((size_t)nt * NBK, 0);
  run([&](int t) {
    int64_t* hh = &hist[(size_t)t * NBK];
    for (int64_t i = n * t / nt; i < n * (t + 1) / nt; ++i)
      ++hh[bucket(a[i])];
  });
  int bs = 0;
  int64_t before = 0;
  for (; bs < NBK; ++bs)
  {
    int64_t c = 0;
    for (int t = 0; t < nt; ++t)
      c += hist[(size_t)t * NBK + bs];
    if (before + c > nl)
      break;
    before += c;
  }
  if (bs == NBK) // nl == n: nothing to split
    return;
  // the nl-th smallest element lives in bucket bs (buckets are ordered by the coordinate)
  std::vector<TileItem> cand;
  for (int64_t i = 0; i < n; ++i)
    if (bucket(a[i]) == bs)
      cand.push_back(a[i]);
  std::nth_element(cand.begin(), cand.begin() + (nl - before), cand.end(),
                   [axis](const TileItem& p, const TileItem& q) { return rcb_less(p, q, axis); });
  const TileItem piv = cand[(size_t)(nl - before)];
  // counting partition: [elements below the splitter | the rest]
  std::vector<int64_t> cnt((size_t)nt + 1, 0);
  run([&](int t) {
    int64_t c = 0;
    for (int64_t i = n * t / nt; i < n * (t + 1) / nt; ++i)
      c += rcb_less(a[i], piv, axis) ? 1 : 0;
    cnt[(size_t)t + 1] = c;
  });
  for (int t = 0; t < nt; ++t)
    cnt[(size_t)t + 1] += cnt[(size_t)t];
  if ((int64_t)tmp.size() < n)
    tmp.resize((size_t)n);
  run([&](int t) {
    const int64_t b = n * t / nt, e = n * (t + 1) / nt;
    int64_t l = cnt[(size_t)t], r = nl + (b - cnt[(size_t)t]);
    for (int64_t i = b; i < e; ++i)
    {
      if (rcb_less(a[i], piv, axis))
        tmp[(size_t)l++] = a[i];
      else
        tmp[(size_t)r++] = a[i];
    }
  });
  run([&](int t) {
    const int64_t b = n * t / nt, e = n * (t + 1) / nt;
    std::copy(tmp.begin() + b, tmp.begin() + e, a + b);
  });
}

static void rcb_partition(TileItem* a, int64_t n, int64_t nl, int axis)
{
  if (axis == 0)
    std::nth_element(a, a + nl, a + n, [](const TileItem& p, const TileItem& q) {
      return p.x < q.x || (p.x == q.x && p.cell < q.cell);
    });
  else
    std::nth_element(a, a + nl, a + n, [](const TileItem& p, const TileItem& q) {
      return p.y < q.y || (p.y == q.y && p.cell < q.cell);
    });
}

// nodes with cells on both sides of the partition [0, nl) | [nl, n): their patches are solved twice
static int64_t rcb_cut_nodes(const TileItem* a, int64_t n, int64_t nl, RcbCtx& c)
{
  const int64_t ep = ++c.epoch;
  int64_t ncut = 0;
  for (int64_t i = 0; i < n; ++i)
  {
    const int64_t tag = 2 * ep + (i < nl ? 0 : 1);
    const int32_t* cn = c.cell_nodes + 3 * (size_t)a[i].cell;
    for (int j = 0; j < 3; ++j)
    {
      int64_t& st = c.stamp[cn[j]];
      if (st / 2 == ep && st != tag && c.cut[cn[j]] != ep)
      {
        c.cut[cn[j]] = ep;
        ++ncut;
      }
      st = tag;
    }
  }
  return ncut;
}

// pool of bisection contexts for the worker threads (a context is [nnodes]-sized)
struct RcbPool
{
  const int32_t* cell_nodes;
  int32_t nnodes;
  const uint8_t* stretched = nullptr; // [ncells] 1: longest edge^2 > 6 |det J| (aspect ratio above ~3)
  std::mutex mtx;
  std::vector<std::unique_ptr<RcbCtx>> free_list;
  std::unique_ptr<RcbCtx> acquire()
  {
    {
      std::lock_guard<std::mutex> g(mtx);
      if (!free_list.empty())
      {
        auto c = std::move(free_list.back());
        free_list.pop_back();
        return c;
      }
    }
    return std::unique_ptr<RcbCtx>(new RcbCtx{cell_nodes, std::vector<int64_t>(nnodes, -1), std::vector<int64_t>(nnodes, -1), 0});
  }
  void release(std::unique_ptr<RcbCtx> c)
  {
    std::lock_guard<std::mutex> g(mtx);
    free_list.push_back(std::move(c));
  }
};

// The subtrees are independent of one another (a context only remembers the nodes of ITS current cut), so
// the upper levels hand their halves to other host threads: same tiles as the serial recursion.
void rcb_split(TileItem* a, int64_t n, int64_t ntile, int tc, RcbPool& pool, RcbCtx* c, int depth)
{
  if (ntile <= 1 || n <= tc)
    return;
  float lo[2] = {3e38f, 3e38f}, hi[2] = {-3e38f, -3e38f};
  int64_t nstretched = 0;
  const bool last_levels = ntile <= 64;
  for (int64_t i = 0; i < n; ++i)
  {
    lo[0] = std::min(lo[0], a[i].x);
    hi[0] = std::max(hi[0], a[i].x);
    lo[1] = std::min(lo[1], a[i].y);
    hi[1] = std::max(hi[1], a[i].y);
    if (last_levels && pool.stretched)
      nstretched += pool.stretched[a[i].cell];
  }
  const int64_t tl = ntile / 2;
  const int64_t nl = std::min<int64_t>(n, tl * tc);
  int axis = (hi[0] - lo[0] >= hi[1] - lo[1]) ? 0 : 1;
  // the last levels decide the shape of the tiles: there the cut is chosen by what it costs - the
  // nodes it separates - not by the extent of the bounding box (which misleads on stretched cells:
  // boundary layers, polar meshes)
  // (where the cells of the segment are not stretched - fewer than 2 % with an aspect ratio above ~3 - the longer
  //  side of the bounding box IS the cheaper cut, and the two trial partitions with their node counts, which
  //  dominated the set-up time of isotropic meshes, are skipped)
  std::unique_ptr<RcbCtx> own;
  if (last_levels && nstretched * 50 > n)
  {
    if (!c)
    {
      own = pool.acquire();
      c = own.get();
    }
    rcb_partition(a, n, nl, axis);
    const int64_t c0 = rcb_cut_nodes(a, n, nl, *c);
    std::vector<TileItem> first(a, a + n); // the partition along `axis`, in case it wins
    rcb_partition(a, n, nl, 1 - axis);
    const int64_t c1 = rcb_cut_nodes(a, n, nl, *c);
    if (c1 < c0)
      axis = 1 - axis; // already partitioned along it
    else
      std::copy(first.begin(), first.end(), a);
  }
  else if (n >= (1 << 18) && depth <= 2) // the top of the tree: few segments, many idle cores
  {
    std::vector<TileItem> tmp;
    rcb_partition_parallel(a, n, nl, axis, lo[axis], hi[axis], tmp);
  }
  else
    rcb_partition(a, n, nl, axis);
  constexpr int PAR_DEPTH = 5; // up to 32 concurrent subtrees
  if (depth < PAR_DEPTH && n > 16 * (int64_t)tc)
  {
    // (a context taken above stays with this thread's half)
    auto left = std::async(std::launch::async, [&]() { rcb_split(a, nl, tl, tc, pool, nullptr, depth + 1); });
    rcb_split(a + nl, n - nl, ntile - tl, tc, pool, c, depth + 1);
    left.get();
  }
  else
  {
    rcb_split(a, nl, tl, tc, pool, c, depth + 1);
    rcb_split(a + nl, n - nl, ntile - tl, tc, pool, c, depth + 1);
  }
  if (own)
    pool.release(std::move(own));
}

// f(i) for i in [0, n) on the host threads (contiguous chunks)
template <typename F>
void parallel_for(int64_t n, int64_t min_chunk, F f)
{
  const int64_t nt = host_workers(n / std::max<int64_t>(min_chunk, 1));
  if (nt <= 1)
  {
    for (int64_t i = 0; i < n; ++i)
      f(i);
    return;
  }
  Workers w;
  for (int64_t t = 0; t < nt; ++t)
    w.spawn([=]() {
      for (int64_t i = n * t / nt; i < n * (t + 1) / nt; ++i)
        f(i);
    });
  w.join();
}

// Wave-blocks per bin and body instance that the tiled kernel of this handle runs over all tiles (eqlb_se_tiling_blocks):
// the split of a tile's list by k_se_stress_tiled (h->t_stress; full_only: lists of full patches, padded) or
// k_se_patch_tiled*, through the range functions the kernels call (eqlb_internal.h)
void count_tile_blocks(eqlb_se* h, const std::vector<eqlb::TileDesc>& tiles, bool full_only)
{
  int64_t* out = h->t_blocks;
  std::fill(out, out + EQLB_TB_COUNT, int64_t(0));
  const int K = h->k;
  for (const eqlb::TileDesc& td : tiles)
  {
    out[EQLB_TB_ZERO_TILES] += td.zero ? 1 : 0;
    for (int b = 0; b < eqlb::MAX_BINS; ++b)
    {
      const int P = eqlb::BIN_P[b];
      int64_t* o = out + EQLB_TB_PER_BIN * b;
      if (h->t_stress)
      {
        if (b >= 2)
          continue; // the fused kernel takes the bins 0, 1
        if (full_only)
        {
          o[EQLB_TB_FULL] += eqlb::tile_wb_whole(td.npatch[b], P);
          o[EQLB_TB_PADDING] += td.npatch[b] - td.nint[b];
          continue;
        }
        const int nwb = eqlb::tile_wb_all(td.npatch[b], P), nwb_full = eqlb::tile_wb_whole(td.nfull[b], P);
        int c0[3], c1[3];
        for (int j = 0; j < 3; ++j)
          if (b == 0)
            eqlb::tile_nfix_range<4>(td, 0, j, c0[j], c1[j]);
          else
            eqlb::tile_nfix_range<8>(td, 1, j, c0[j], c1[j]);
        int nfix = 0;
        for (int j = 0; j < 3; ++j)
        {
          o[EQLB_TB_NFIX1 + j] += c1[j] - c0[j];
          nfix += c1[j] - c0[j];
        }
        o[EQLB_TB_FULL] += nwb_full;
        o[EQLB_TB_GENERIC] += nwb - nwb_full - nfix;
        continue;
      }
      const int nwb = eqlb::tile_wb_all(td.npatch[b], P);
      const int nwb_full = eqlb::tile_spec_full(K, P) ? eqlb::tile_wb_whole(td.nfull[b], P) : 0;
      const int nwb_int = eqlb::tile_spec_interior(K, P) ? eqlb::tile_wb_whole(td.nint[b], P) : 0;
      const int nint = std::max(nwb_int - nwb_full, 0); // (k_se_patch_tiled: u < nwb_full first, then u < nwb_int)
      o[EQLB_TB_FULL] += nwb_full;
      o[EQLB_TB_INTERIOR] += nint;
      o[EQLB_TB_GENERIC] += nwb - nwb_full - nint;
    }
  }
}
} // namespace

namespace eqlb
{
// Tiled SoA of the plain flux equilibration (EQLB_SCATTER_TILED): cells bisected recursively by
// their centroids into tiles of TC cells; a tile lists every (masked-in) node of its cells.
int build_tiles(eqlb_se* h, const std::vector<int8_t>& node_bin_all, eqlb::BuildArgs a, int tc_fixed, int max_bin,
                bool full_only)
{
  // nodes of bins >= max_bin are left out (like masked-out nodes): another path equilibrates them.
  // full_only (fused stress launch on the crossed benchmark meshes): so are all patches that are not FULL (interior,
  // as many cells as lanes); the lists of a tile are padded to whole wave-blocks with copies of a full patch that
  // own no cell
  const eqlb::DeviceMesh& m = h->mesh->m;
  const int32_t nc = m.ncells;
  std::vector<int8_t> node_bin(node_bin_all);
  std::vector<uint8_t> is_rest(max_bin < eqlb::MAX_BINS ? m.nnodes : 0, 0);
  h->t_rest = 0;
  for (int32_t i = 0; i < m.nnodes; ++i)
  {
    int8_t& b = node_bin[i];
    if (b < 0)
      continue;
    const bool full = m.h_node_ncells[i] == m.h_node_nfcts[i] && m.h_node_ncells[i] == eqlb::BIN_P[b];
    if (b >= max_bin || (full_only && !full))
    {
      b = -1;
      ++h->t_rest;
      if (!is_rest.empty())
        is_rest[i] = 1;
    }
  }
  dfree(h->rest_cells);
  h->nrest_cells = 0;
  if (!is_rest.empty() && h->t_rest > 0)
  {
    // cells with a vertex whose patch the generic kernels take: the compact reduction of their slot rows
    std::vector<int32_t> rc;
    for (int32_t c = 0; c < nc; ++c)
      for (int j = 0; j < 3; ++j)
      {
        const int32_t nd = m.h_cell_nodes[3 * (size_t)c + j];
        if (is_rest[nd])
        {
          rc.push_back(c);
          break;
        }
      }
    h->nrest_cells = (int64_t)rc.size();
    if (upload(&h->rest_cells, rc.data(), std::max<size_t>(rc.size(), 1)))
      return EQLB_ERR_DEVICE;
  }
  // Tile size: the default, or - on meshes that fill the chip several times over - the size that
  // makes the tiles fill whole rounds of the 512 workgroup slots (2 per CU): 1M triangles in 2 045
  // tiles of 489 cells run in 4 rounds, 2 084 tiles of 480 cells leave 36 tiles for a fifth
  int TC = tc_fixed > 0 ? tc_fixed : eqlb::tile_cells_of(h->k);
  if (tc_fixed > 0)
  {
    // fused stress launch (tc_fixed = the largest tile its LDS holds): ONE workgroup per CU, so a partial last
    // round of the 256 slots costs a full round - fit the tile size to whole rounds as below
    const int64_t slots = 256, tcmax = tc_fixed;
    TC = (int)std::min<int64_t>(tcmax, 448);
    if ((int64_t)nc >= slots * 256)
    {
      const int64_t rounds = ((int64_t)nc + slots * tcmax - 1) / (slots * tcmax);
      TC = (int)(((int64_t)nc + rounds * slots - 1) / (rounds * slots));
    }
    if (h->tile_cells_user > 0)
      TC = (int)std::min<int64_t>(h->tile_cells_user, tcmax);
  }
  if (tc_fixed <= 0)
  {
    // resident workgroup slots of the chip: two per CU for k <= 2, one for k = 3
    const bool ev3 = h->mode == 1 && h->k >= 3; // EV mode of RT_3 stages 7 KB more tensors: smaller tiles
    const int64_t slots = (h->k <= 2) ? 512 : 256, tcmax = ev3 ? eqlb::tile_cells_ev_of(h->k) : eqlb::tile_cells_max_of(h->k);
    if (ev3)
      TC = eqlb::tile_cells_ev_of(h->k);
    if ((int64_t)nc >= slots * 256)
    {
      const int64_t rounds = ((int64_t)nc + slots * tcmax - 1) / (slots * tcmax);
      TC = (int)(((int64_t)nc + rounds * slots - 1) / (rounds * slots));
    }
    if (h->tile_cells_user > 0) // tuning knob (option "tile_cells"), capped by what the LDS of a workgroup holds
      TC = (int)std::min<int64_t>(h->tile_cells_user, tcmax);
  }
  SetupTimer tm;
  uvec<TileItem> items(nc);
  const int32_t ntiles = (nc + TC - 1) / TC;
  bool cached = false;
  {
    std::lock_guard<std::mutex> g(h->mesh->tiling_mutex);
    auto it = h->mesh->tiling_order.find(TC);
    if (it != h->mesh->tiling_order.end() && (int32_t)it->second.size() == nc)
    {
      for (int32_t p = 0; p < nc; ++p)
        items[p] = {0.0f, 0.0f, it->second[p]};
      cached = true;
    }
  }
  if (!cached)
  {
  std::vector<uint8_t> stretched(nc);
  // bounding box of the nodes: the centroids are stored relative to it (one scale for both directions)
  double blo[2] = {1e300, 1e300}, bhi[2] = {-1e300, -1e300};
  for (int32_t i = 0; i < m.nnodes; ++i)
    for (int d = 0; d < 2; ++d)
    {
      blo[d] = std::min(blo[d], m.h_x[3 * (size_t)i + d]);
      bhi[d] = std::max(bhi[d], m.h_x[3 * (size_t)i + d]);
    }
  const double ext = std::max(bhi[0] - blo[0], bhi[1] - blo[1]);
  const double inv = (ext > 0.0) ? 1.0 / (3.0 * ext) : 0.0;
  // the bisection on the device (one radix sort per level of the tree; eqlb_tiling_device.hip) unless the mesh
  // has stretched cells, where the host bisection below picks the cuts of the last levels by their cost
  bool on_device = false;
  {
    const char* env = getenv("EQLB_TILING");
    if (!(env && !strcmp(env, "host")) && nc >= 4096)
    {
      std::vector<int32_t> dord;
      const int r = eqlb::device_tile_order(m, TC, ntiles, blo, bhi, inv, dord);
      if (r < 0)
        return fail(EQLB_ERR_DEVICE, "tiling on the device failed");
      if (r == 0)
      {
        for (int32_t p = 0; p < nc; ++p)
          items[p] = {0.0f, 0.0f, dord[p]};
        on_device = true;
        tm.lap("tiles: bisection (device)");
      }
    }
  }
  if (!on_device)
  {
  parallel_for(nc, 1 << 16, [&](int64_t c) {
    const int32_t* cn = &m.h_cell_nodes[3 * (size_t)c];
    double cx = 0.0, cy = 0.0;
    for (int j = 0; j < 3; ++j)
    {
      cx += m.h_x[3 * (size_t)cn[j]] - blo[0];
      cy += m.h_x[3 * (size_t)cn[j] + 1] - blo[1];
    }
    items[c] = {(float)(cx * inv), (float)(cy * inv), (int32_t)c};
    const double* p0 = &m.h_x[3 * (size_t)cn[0]];
    const double* p1 = &m.h_x[3 * (size_t)cn[1]];
    const double* p2 = &m.h_x[3 * (size_t)cn[2]];
    const double e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e2x = p2[0] - p0[0], e2y = p2[1] - p0[1];
    const double l2 = std::max(std::max(e1x * e1x + e1y * e1y, e2x * e2x + e2y * e2y),
                               (e2x - e1x) * (e2x - e1x) + (e2y - e1y) * (e2y - e1y));
    stretched[c] = l2 > 6.0 * std::fabs(e1x * e2y - e1y * e2x) ? 1 : 0;
  });
  RcbPool pool{m.h_cell_nodes.data(), m.nnodes, stretched.data(), {}, {}};
  tm.lap("tiles: centroids");
  rcb_split(items.data(), nc, ntiles, TC, pool, nullptr, 0);
  tm.lap("tiles: bisection");
  // ascending cell ids inside a tile: the flush of a tile then touches flux_hdiv in long runs
  parallel_for(ntiles, 16, [&](int64_t t) {
    std::sort(items.begin() + (size_t)t * TC, items.begin() + std::min<size_t>((size_t)(t + 1) * TC, nc),
              [](const TileItem& p, const TileItem& q) { return p.cell < q.cell; });
  });
  }
  std::vector<int32_t> ord(nc);
  for (int32_t p = 0; p < nc; ++p)
    ord[p] = items[p].cell;
  std::lock_guard<std::mutex> g(h->mesh->tiling_mutex);
  h->mesh->tiling_order[TC] = std::move(ord);
  }
  // tiles that own a priority cell (ghost rows a neighbour rank waits for) are numbered first: a
  // first launch over them, the halo exchange, and the launch over the rest then overlap
  std::vector<int32_t> order(ntiles);
  {
    std::vector<uint8_t> tile_prio(ntiles, 0);
    if (!h->prio_cells.empty())
    {
      std::vector<uint8_t> is_prio(nc, 0);
      for (int32_t c : h->prio_cells)
        if (c >= 0 && c < nc)
          is_prio[c] = 1;
      for (int32_t p = 0; p < nc; ++p)
        if (is_prio[items[p].cell])
          tile_prio[p / TC] = 1;
    }
    int32_t np = 0;
    for (int32_t t = 0; t < ntiles; ++t)
      if (tile_prio[t])
        order[np++] = t;
    h->t_nprio = np;
    for (int32_t t = 0; t < ntiles; ++t)
      if (!tile_prio[t])
        order[np++] = t;
  }
  tm.lap("tiles: sort + priority");
  uvec<int32_t> tile_cells((size_t)ntiles * TC), cell_tile(nc), cell_pos(nc);
  parallel_for(ntiles, 16, [&](int64_t t) {
    const int64_t src = (int64_t)order[t] * TC, len = std::min<int64_t>(TC, nc - src);
    for (int64_t q = 0; q < len; ++q)
    {
      const int32_t c = items[src + q].cell;
      tile_cells[(size_t)t * TC + q] = c;
      cell_tile[c] = (int32_t)t;
      cell_pos[c] = (int32_t)((int64_t)t * TC + q);
    }
    for (int64_t q = len; q < TC; ++q)
      tile_cells[(size_t)t * TC + q] = -1;
  });
  std::vector<eqlb::TileDesc> tiles(ntiles);
  // pass 1 (host threads, a chunk of tiles each): the nodes of every tile by bin - full interior patches
  // (as many cells as lanes, no boundary facet: their wave-blocks run the specialised body of the kernel)
  // first -, in order of first appearance; flat storage, 3 TC entries per tile
  constexpr int NB = eqlb::MAX_BINS;
  uvec<int32_t> tnodes((size_t)ntiles * 3 * TC);
  constexpr int NCL = 6; // classes of a bin: full | interior with P - 1, P - 2, P - 3 cells | other interior | boundary
  std::vector<int32_t> tcount((size_t)ntiles * NCL * NB, 0); // [tile][bin][class]
  auto tile_chunks = [&](auto work) {
    const int64_t nt = host_workers(ntiles / 32);
    if (nt <= 1)
    {
      work(0, ntiles);
      return;
    }
    Workers wk;
    for (int64_t w = 0; w < nt; ++w)
      wk.spawn([&work, ntiles, w, nt]() { work((int64_t)ntiles * w / nt, (int64_t)ntiles * (w + 1) / nt); });
    wk.join();
  };
  // sort key of a node: NCL * bin + class (full interior patch 0 | interior patch with P - 1, P - 2, P - 3 cells 1, 2, 3 |
  // other interior patch 4 | boundary patch 5); -1: not listed
  // (one byte per node, cache resident, instead of three scattered reads per visit of a node)
  std::vector<int8_t> nkey(m.nnodes);
  parallel_for(m.nnodes, 1 << 16, [&](int64_t nd) {
    const int b_ = node_bin[nd];
    if (b_ < 0)
    {
      nkey[nd] = -1;
      return;
    }
    const bool interior = m.h_node_ncells[nd] == m.h_node_nfcts[nd]; // no boundary facet at the node
    const int missing = eqlb::BIN_P[b_] - m.h_node_ncells[nd];         // idle lanes of the patch group
    nkey[nd] = (int8_t)(NCL * b_ + (interior ? ((missing >= 0 && missing <= 3) ? missing : 4) : 5));
  });
  tile_chunks([&](int64_t t0, int64_t t1) {
    std::vector<int32_t> stamp(m.nnodes, -1), seen(3 * (size_t)TC);
    for (int64_t t = t0; t < t1; ++t)
    {
      int nseen = 0;
      int32_t* cnt = &tcount[(size_t)t * NCL * NB];
      auto key = [&](int32_t nd) { return (int)nkey[nd]; };
      for (int q = 0; q < TC; ++q)
      {
        const int32_t c = tile_cells[(size_t)t * TC + q];
        if (c < 0)
          continue;
        for (int j = 0; j < 3; ++j)
        {
          const int32_t nd = m.h_cell_nodes[3 * (size_t)c + j];
          if (nkey[nd] < 0)
            tiles[t].zero = 1; // masked-out vertex: the (cell, vertex) row of this tile stays unwritten
          if (nkey[nd] < 0 || stamp[nd] == (int32_t)t)
            continue;
          stamp[nd] = (int32_t)t;
          seen[nseen++] = nd;
          ++cnt[key(nd)];
        }
      }
      int32_t pos[NCL * NB], acc = 0; // stable counting sort by (bin, class)
      for (int q = 0; q < NCL * NB; ++q)
      {
        pos[q] = acc;
        acc += cnt[q];
      }
      int32_t* out = &tnodes[(size_t)t * 3 * TC];
      for (int i = 0; i < nseen; ++i)
        out[pos[key(seen[i])]++] = seen[i];
      for (int b_ = 0; b_ < NB; ++b_)
      {
        const int32_t* cb = cnt + NCL * b_;
        tiles[t].nfull[b_] = cb[0];
        tiles[t].nint[b_] = cb[0] + cb[1] + cb[2] + cb[3] + cb[4];
        tiles[t].npatch[b_] = tiles[t].nint[b_] + cb[5];
        if (b_ < 2)
        {
          tiles[t].nval[b_][0] = cb[0] + cb[1];
          tiles[t].nval[b_][1] = cb[0] + cb[1] + cb[2];
          tiles[t].nval[b_][2] = cb[0] + cb[1] + cb[2] + cb[3];
        }
        if (full_only)
        {
          // whole wave-blocks: nint keeps the number of real patches, the others are copies (pass 2)
          const int per = 64 / eqlb::BIN_P[b_];
          const int padded = (per > 0) ? (cb[0] + per - 1) / per * per : cb[0];
          tiles[t].nfull[b_] = padded;
          tiles[t].npatch[b_] = padded;
          if (b_ < 2)
            tiles[t].nval[b_][0] = tiles[t].nval[b_][1] = tiles[t].nval[b_][2] = padded;
        }
      }
    }
  });
  // lane slots and patch instances in tile order (serial prefix), then filled by the host threads
  int64_t slotctr = 0, ninst = 0;
  for (int32_t t = 0; t < ntiles; ++t)
    for (int b_ = 0; b_ < NB; ++b_)
    {
      tiles[t].slot_start[b_] = (int32_t)slotctr;
      tiles[t].patch_start[b_] = (int32_t)ninst;
      slotctr += (int64_t)tiles[t].npatch[b_] * eqlb::BIN_P[b_];
      ninst += tiles[t].npatch[b_];
      slotctr = (slotctr + 63) & ~(int64_t)63;
      if (slotctr > 0x7fffff00)
        return fail(EQLB_ERR_UNSUPPORTED, "tiled patch SoA exceeds 2^31 lane slots");
    }
  uvec<int32_t> inst_node((size_t)ninst), inst_slot((size_t)ninst), inst_tile((size_t)ninst);
  tile_chunks([&](int64_t t0, int64_t t1) {
    for (int64_t t = t0; t < t1; ++t)
    {
      const int32_t* src = &tnodes[(size_t)t * 3 * TC];
      for (int b_ = 0; b_ < NB; ++b_)
      {
        int32_t slot = tiles[t].slot_start[b_];
        const int32_t nreal = full_only ? tiles[t].nint[b_] : tiles[t].npatch[b_];
        for (int32_t i = 0, p_ = tiles[t].patch_start[b_]; i < tiles[t].npatch[b_]; ++i, ++p_, slot += eqlb::BIN_P[b_])
        {
          // (padding copy: the last real patch once more, tile -1 = it owns no cell and stores nothing)
          inst_node[p_] = (i < nreal) ? *src++ : src[-1];
          inst_slot[p_] = slot;
          inst_tile[p_] = (i < nreal) ? (int32_t)t : -1;
        }
      }
    }
  });
  tm.lap("tiles: patch lists");
  count_tile_blocks(h, tiles, full_only);
  h->ntiles = ntiles;
  h->tile_tc = TC;
  h->t_nslots = slotctr;
  h->t_npatch = (int64_t)inst_node.size();
  int32_t *d_inode = nullptr, *d_islot = nullptr, *d_itile = nullptr, *d_ctile = nullptr, *d_cpos = nullptr;
  int st = 0;
  st |= upload(&h->t_tiles, tiles.data(), tiles.size());
  st |= upload(&h->t_tile_cells, tile_cells.data(), tile_cells.size());
  st |= upload<int32_t>(&h->t_slot_cell, nullptr, (size_t)std::max<int64_t>(slotctr, 1));
  st |= upload<uint32_t>(&h->t_slot_info, nullptr, (size_t)std::max<int64_t>(slotctr, 1));
  st |= upload<uint8_t>(&h->t_pn, nullptr, (size_t)std::max<int64_t>(h->t_npatch, 1));
  st |= upload<uint8_t>(&h->t_pflag, nullptr, (size_t)std::max<int64_t>(h->t_npatch, 1) * h->nrhs);
  st |= upload(&d_inode, inst_node.data(), std::max<size_t>(inst_node.size(), 1));
  st |= upload(&d_islot, inst_slot.data(), std::max<size_t>(inst_slot.size(), 1));
  st |= upload(&d_itile, inst_tile.data(), std::max<size_t>(inst_tile.size(), 1));
  st |= upload(&d_ctile, cell_tile.data(), cell_tile.size());
  st |= upload(&d_cpos, cell_pos.data(), cell_pos.size());
  hipError_t e = hipSuccess;
  if (!st)
  {
    e = hipMemset(h->t_slot_cell, 0xff, sizeof(int32_t) * std::max<int64_t>(slotctr, 1));
    if (e == hipSuccess)
      e = hipMemset(h->t_slot_info, 0, sizeof(uint32_t) * std::max<int64_t>(slotctr, 1));
    a.ninst = h->t_npatch;
    a.inst_node = d_inode;
    a.inst_slot = d_islot;
    a.inst_tile = d_itile;
    a.cell_tile = d_ctile;
    a.cell_pos = d_cpos;
    a.tile_cells = TC;
    a.npatch_total = h->t_npatch;
    a.slot_cell = h->t_slot_cell;
    a.slot_info = h->t_slot_info;
    a.pn = h->t_pn;
    a.pflag = h->t_pflag;
    a.stride = 0;
    a.ex_ncells = nullptr;
    if (e == hipSuccess && a.ninst > 0)
    {
      eqlb::launch_build_patches(a, nullptr);
      e = hipGetLastError();
    }
    if (e == hipSuccess)
      e = hipDeviceSynchronize();
  }
  tm.lap("tiles: upload + builder kernel");
  dfree(d_inode);
  dfree(d_islot);
  dfree(d_itile);
  dfree(d_ctile);
  dfree(d_cpos);
  if (st)
    return EQLB_ERR_DEVICE;
  if (e != hipSuccess)
    return fail(EQLB_ERR_DEVICE, "tiled patch builder: %s", hipGetErrorString(e));
  return EQLB_OK;
}
} // namespace eqlb
