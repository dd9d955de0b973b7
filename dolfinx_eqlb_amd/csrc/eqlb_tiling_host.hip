// Tiles of the tiled launch (EQLB_SCATTER_TILED) on the host: recursive coordinate bisection of the cell centroids
// (rcb_split) and the tiled patch SoA planned from it (plan_tiles, called by eqlb_se_set_boundary before the handle
// changes; eqlb_boundary_setup.hip uploads the plan).  Host code only; the device bisection it tries first is
// eqlb_tiling_device.hip.
#include "eqlb_handle.h"

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

// Host worker threads of the set-up: capped (the tile builder keeps an O(nnodes) stamp per worker: 16 MB each at
// 4M nodes, on every rank of a node) and exception safe - an exception inside a std::thread would call
// std::terminate; the first one is kept and re-thrown by join() in the calling thread, where the C entry points
// turn it into an error code (EQLB_CATCH_ALL).
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

// Wave-blocks per bin and body instance that the tiled kernel runs over all tiles (eqlb_se_tiling_blocks): the split of
// a tile's list by k_se_stress_tiled (t_stress; full_only: lists of full patches, padded) or k_se_patch_tiled*,
// through the range functions the kernels call (eqlb_internal.h)
void count_tile_blocks(int K, bool t_stress, bool full_only, const std::vector<eqlb::TileDesc>& tiles, int64_t* out)
{
  std::fill(out, out + EQLB_TB_COUNT, int64_t(0));
  for (const eqlb::TileDesc& td : tiles)
  {
    out[EQLB_TB_ZERO_TILES] += td.zero ? 1 : 0;
    for (int b = 0; b < eqlb::MAX_BINS; ++b)
    {
      const int P = eqlb::BIN_P[b];
      int64_t* o = out + EQLB_TB_PER_BIN * b;
      if (t_stress)
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

// The cells in the order of the tile bisection, chunks of tc cells with ascending ids inside a chunk: from the cache of
// the mesh, else by the bisection on the device (one radix sort per level of the tree; eqlb_tiling_device.hip) or,
// where the mesh has stretched cells or is small, on the host threads - and then kept in the cache
int bisect_cells(eqlb_mesh* mesh, int tc, int32_t ntiles, SetupTimer& tm, eqlb::uvec<int32_t>& cells)
{
  const eqlb::DeviceMesh& m = mesh->m;
  const eqlb::HostMesh& hm = mesh->host;
  const int32_t nc = m.ncells;
  {
    std::lock_guard<std::mutex> g(mesh->tiling_mutex);
    auto it = mesh->tiling_order.find(tc);
    if (it != mesh->tiling_order.end() && (int32_t)it->second.size() == nc)
    {
      cells.assign(it->second.begin(), it->second.end());
      return EQLB_OK;
    }
  }
  // bounding box of the nodes: the centroids are stored relative to it (one scale for both directions)
  double blo[2] = {1e300, 1e300}, bhi[2] = {-1e300, -1e300};
  for (int32_t i = 0; i < m.nnodes; ++i)
    for (int d = 0; d < 2; ++d)
    {
      blo[d] = std::min(blo[d], hm.x[3 * (size_t)i + d]);
      bhi[d] = std::max(bhi[d], hm.x[3 * (size_t)i + d]);
    }
  const double ext = std::max(bhi[0] - blo[0], bhi[1] - blo[1]);
  const double inv = (ext > 0.0) ? 1.0 / (3.0 * ext) : 0.0;
  std::vector<int32_t> ord;
  const char* env = getenv("EQLB_TILING");
  int on_host = 1;
  if (!(env && !strcmp(env, "host")) && nc >= 4096)
  {
    on_host = eqlb::device_tile_order(m, tc, ntiles, blo, bhi, inv, ord); // 1: stretched mesh
    if (on_host < 0)
      return fail(EQLB_ERR_DEVICE, "tiling on the device failed");
    if (!on_host)
      tm.lap("tiles: bisection (device)");
  }
  if (on_host)
  {
    eqlb::uvec<TileItem> items(nc);
    std::vector<uint8_t> stretched(nc);
    parallel_for(nc, 1 << 16, [&](int64_t c) {
      const int32_t* cn = &hm.cell_nodes[3 * (size_t)c];
      double cx = 0.0, cy = 0.0;
      for (int j = 0; j < 3; ++j)
      {
        cx += hm.x[3 * (size_t)cn[j]] - blo[0];
        cy += hm.x[3 * (size_t)cn[j] + 1] - blo[1];
      }
      items[c] = {(float)(cx * inv), (float)(cy * inv), (int32_t)c};
      const double* p0 = &hm.x[3 * (size_t)cn[0]];
      const double* p1 = &hm.x[3 * (size_t)cn[1]];
      const double* p2 = &hm.x[3 * (size_t)cn[2]];
      const double e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e2x = p2[0] - p0[0], e2y = p2[1] - p0[1];
      const double l2 = std::max(std::max(e1x * e1x + e1y * e1y, e2x * e2x + e2y * e2y),
                                 (e2x - e1x) * (e2x - e1x) + (e2y - e1y) * (e2y - e1y));
      stretched[c] = l2 > 6.0 * std::fabs(e1x * e2y - e1y * e2x) ? 1 : 0;
    });
    RcbPool pool{hm.cell_nodes.data(), m.nnodes, stretched.data(), {}, {}};
    tm.lap("tiles: centroids");
    rcb_split(items.data(), nc, ntiles, tc, pool, nullptr, 0);
    tm.lap("tiles: bisection");
    // ascending cell ids inside a tile: the flush of a tile then touches flux_hdiv in long runs
    parallel_for(ntiles, 16, [&](int64_t t) {
      std::sort(items.begin() + (size_t)t * tc, items.begin() + std::min<size_t>((size_t)(t + 1) * tc, nc),
                [](const TileItem& p, const TileItem& q) { return p.cell < q.cell; });
    });
    ord.resize(nc);
    for (int32_t p = 0; p < nc; ++p)
      ord[p] = items[p].cell;
  }
  cells.assign(ord.begin(), ord.end());
  std::lock_guard<std::mutex> g(mesh->tiling_mutex);
  mesh->tiling_order[tc] = std::move(ord);
  return EQLB_OK;
}

// Tiles that own a priority cell (ghost rows a neighbour rank waits for) are numbered first: a first launch over them,
// the halo exchange, and the launch over the rest then overlap.  Fills the cell tables of the tiles in that numbering.
void number_tiles(const std::vector<int32_t>& prio_cells, int32_t nc, const eqlb::uvec<int32_t>& cells,
                  eqlb::TilePlan& tp)
{
  const int32_t ntiles = tp.ntiles, TC = tp.tc;
  std::vector<int32_t> order(ntiles);
  std::vector<uint8_t> tile_prio(ntiles, 0);
  if (!prio_cells.empty())
  {
    std::vector<uint8_t> is_prio(nc, 0);
    for (int32_t c : prio_cells)
      if (c >= 0 && c < nc)
        is_prio[c] = 1;
    for (int32_t p = 0; p < nc; ++p)
      if (is_prio[cells[p]])
        tile_prio[p / TC] = 1;
  }
  int32_t np = 0;
  for (int32_t t = 0; t < ntiles; ++t)
    if (tile_prio[t])
      order[np++] = t;
  tp.nprio = np;
  for (int32_t t = 0; t < ntiles; ++t)
    if (!tile_prio[t])
      order[np++] = t;
  tp.tile_cells.resize((size_t)ntiles * TC);
  tp.cell_tile.resize(nc);
  tp.cell_pos.resize(nc);
  parallel_for(ntiles, 16, [&](int64_t t) {
    const int64_t src = (int64_t)order[t] * TC, len = std::min<int64_t>(TC, nc - src);
    for (int64_t q = 0; q < len; ++q)
    {
      const int32_t c = cells[src + q];
      tp.tile_cells[(size_t)t * TC + q] = c;
      tp.cell_tile[c] = (int32_t)t;
      tp.cell_pos[c] = (int32_t)((int64_t)t * TC + q);
    }
    for (int64_t q = len; q < TC; ++q)
      tp.tile_cells[(size_t)t * TC + q] = -1;
  });
}

// work(t0, t1) on chunks of tiles, one per host thread
template <typename F>
void tile_chunks(int32_t ntiles, F work)
{
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
}

constexpr int NB = eqlb::MAX_BINS;
constexpr int NCL = 6; // classes of a bin: full | interior with P - 1, P - 2, P - 3 cells | other interior | boundary

// Pass 1 (host threads, a chunk of tiles each): the listed nodes of every tile by bin and class - full interior
// patches (their wave-blocks run the specialised body of the kernel) first -, in order of first appearance; tnodes:
// flat storage, 3 TC entries per tile.  full_only: the lists of a tile are padded to whole wave-blocks with copies of
// a full patch that own no cell (nint keeps the number of real patches)
void list_tile_patches(const eqlb::HostMesh& m, const std::vector<int8_t>& tile_bin, bool full_only,
                       eqlb::TilePlan& tp, eqlb::uvec<int32_t>& tnodes)
{
  const int TC = tp.tc;
  const size_t nnodes = m.node_ncells.size();
  std::vector<eqlb::TileDesc>& tiles = tp.tiles;
  // sort key of a node: NCL * bin + class (full interior patch 0 | interior patch with P - 1, P - 2, P - 3 cells 1, 2, 3 |
  // other interior patch 4 | boundary patch 5); -1: not listed
  // (one byte per node, cache resident, instead of three scattered reads per visit of a node)
  std::vector<int8_t> nkey(nnodes);
  parallel_for(nnodes, 1 << 16, [&](int64_t nd) {
    const int b_ = tile_bin[nd];
    if (b_ < 0)
    {
      nkey[nd] = -1;
      return;
    }
    const bool interior = m.node_ncells[nd] == m.node_nfcts[nd]; // no boundary facet at the node
    const int missing = eqlb::BIN_P[b_] - m.node_ncells[nd];         // idle lanes of the patch group
    const int cls = eqlb::patch_is_full(m.node_ncells[nd], m.node_nfcts[nd], b_) ? 0
                    : !interior                                                       ? 5
                    : (missing >= 1 && missing <= 3)                                  ? missing
                                                                                      : 4;
    nkey[nd] = (int8_t)(NCL * b_ + cls);
  });
  tile_chunks(tp.ntiles, [&](int64_t t0, int64_t t1) {
    std::vector<int32_t> stamp(nnodes, -1), seen(3 * (size_t)TC);
    for (int64_t t = t0; t < t1; ++t)
    {
      int nseen = 0;
      int32_t cnt[NCL * NB] = {};
      for (int q = 0; q < TC; ++q)
      {
        const int32_t c = tp.tile_cells[(size_t)t * TC + q];
        if (c < 0)
          continue;
        for (int j = 0; j < 3; ++j)
        {
          const int32_t nd = m.cell_nodes[3 * (size_t)c + j];
          if (nkey[nd] < 0)
            tiles[t].zero = 1; // masked-out vertex: the (cell, vertex) row of this tile stays unwritten
          if (nkey[nd] < 0 || stamp[nd] == (int32_t)t)
            continue;
          stamp[nd] = (int32_t)t;
          seen[nseen++] = nd;
          ++cnt[nkey[nd]];
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
        out[pos[nkey[seen[i]]]++] = seen[i];
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
          // whole wave-blocks: nint keeps the number of real patches, the others are copies (place_instances)
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
}

// Lane slots and patch instances in tile order (serial prefix), then filled by the host threads
int place_instances(bool full_only, const eqlb::uvec<int32_t>& tnodes, eqlb::TilePlan& tp)
{
  std::vector<eqlb::TileDesc>& tiles = tp.tiles;
  int64_t slotctr = 0, ninst = 0;
  for (int32_t t = 0; t < tp.ntiles; ++t)
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
  tp.nslots = slotctr;
  tp.inst_node.resize((size_t)ninst);
  tp.inst_slot.resize((size_t)ninst);
  tp.inst_tile.resize((size_t)ninst);
  tile_chunks(tp.ntiles, [&](int64_t t0, int64_t t1) {
    for (int64_t t = t0; t < t1; ++t)
    {
      const int32_t* src = &tnodes[(size_t)t * 3 * tp.tc];
      for (int b_ = 0; b_ < NB; ++b_)
      {
        int32_t slot = tiles[t].slot_start[b_];
        const int32_t nreal = full_only ? tiles[t].nint[b_] : tiles[t].npatch[b_];
        for (int32_t i = 0, p_ = tiles[t].patch_start[b_]; i < tiles[t].npatch[b_]; ++i, ++p_, slot += eqlb::BIN_P[b_])
        {
          // (padding copy: the last real patch once more, tile -1 = it owns no cell and stores nothing)
          tp.inst_node[p_] = (i < nreal) ? *src++ : src[-1];
          tp.inst_slot[p_] = slot;
          tp.inst_tile[p_] = (i < nreal) ? (int32_t)t : -1;
        }
      }
    }
  });
  return EQLB_OK;
}
} // namespace

namespace eqlb
{
// Tiled SoA of the plain flux equilibration (EQLB_SCATTER_TILED) and of the fused stress launch: cells bisected
// recursively by their centroids into tiles of TC cells; a tile lists every node of its cells that bp.tile_bin lists
// (not the masked-out ones, not those left to another path)
int plan_tiles(const eqlb_se* h, const BoundaryPlan& bp, TilePlan& tp)
{
  const DeviceMesh& m = h->mesh->m;
  const bool full_only = bp.t_stress && !bp.t_mixed;
  tp.tc = choose_tile_cells(h->k, h->mode, m.ncells, bp.t_stress ? stress_tile_cells() : 0, h->tile_cells_user,
                            {tile_cells_of(h->k), tile_cells_ev_of(h->k), tile_cells_max_of(h->k)});
  tp.ntiles = (m.ncells + tp.tc - 1) / tp.tc;
  SetupTimer tm;
  uvec<int32_t> cells;
  EQLB_TRY(bisect_cells(h->mesh, tp.tc, tp.ntiles, tm, cells));
  number_tiles(h->prio_cells, m.ncells, cells, tp);
  tm.lap("tiles: sort + priority");
  tp.tiles.assign(tp.ntiles, TileDesc{});
  uvec<int32_t> tnodes((size_t)tp.ntiles * 3 * tp.tc);
  list_tile_patches(h->mesh->host, bp.tile_bin, full_only, tp, tnodes);
  EQLB_TRY(place_instances(full_only, tnodes, tp));
  tm.lap("tiles: patch lists");
  count_tile_blocks(h->k, bp.t_stress, full_only, tp.tiles, tp.blocks);
  return EQLB_OK;
}
} // namespace eqlb
