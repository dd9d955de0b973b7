// The host predicates of dolfinx_eqlb_amd/csrc/eqlb_topology_check.h - which nodes the patch builder can walk, which
// facet-type tables eqlb_se_set_boundary refuses - on small meshes written down here, with the verdict and the named
// node / facet of each checked.
//
//   c++ -O1 -g -std=c++17 [-fsanitize=address,undefined] tools/topology_check_emul.cpp -o topology_check_emul
//   ./topology_check_emul
//
// exit status 0 and "PASS": every table gave the expected verdict.  No GPU, no HIP.
//
// The meshes are lists of triangles; facets are numbered in order of first appearance (cell by cell, local edges
// (0,1), (1,2), (2,0)), and the tables the header reads are counted from them without any use of the header.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <utility>
#include <vector>

#include "../dolfinx_eqlb_amd/csrc/eqlb_topology_check.h"

namespace
{
struct Mesh
{
  int32_t nnodes = 0, nfacets = 0;
  std::vector<int32_t> cells;                       // [ncells][3]
  std::vector<int32_t> facet_nodes, facet_cells_off; // [nfacets][2], [nfacets + 1]
  std::vector<int32_t> node_facets_off, node_facets; // CSR
  std::vector<int32_t> node_ncells, node_nfcts;
  std::map<std::pair<int32_t, int32_t>, int32_t> fid;

  int32_t facet(int32_t a, int32_t b) const { return fid.at({std::min(a, b), std::max(a, b)}); }
  bool boundary(int32_t f) const { return facet_cells_off[f + 1] - facet_cells_off[f] == 1; }
};

Mesh make_mesh(int32_t nnodes, const std::vector<int32_t>& cells)
{
  Mesh m;
  m.nnodes = nnodes;
  m.cells = cells;
  std::vector<int32_t> fcells; // cells per facet
  m.node_ncells.assign(nnodes, 0);
  for (size_t c = 0; c < cells.size() / 3; ++c)
    for (int e = 0; e < 3; ++e)
    {
      const int32_t a = cells[3 * c + e], b = cells[3 * c + (e + 1) % 3];
      const std::pair<int32_t, int32_t> key{std::min(a, b), std::max(a, b)};
      auto it = m.fid.find(key);
      if (it == m.fid.end())
      {
        it = m.fid.emplace(key, (int32_t)fcells.size()).first;
        fcells.push_back(0);
        m.facet_nodes.push_back(key.first);
        m.facet_nodes.push_back(key.second);
      }
      ++fcells[it->second];
      ++m.node_ncells[a];
    }
  m.nfacets = (int32_t)fcells.size();
  m.facet_cells_off.assign(1, 0);
  for (int32_t f = 0; f < m.nfacets; ++f)
    m.facet_cells_off.push_back(m.facet_cells_off.back() + fcells[f]);
  m.node_nfcts.assign(nnodes, 0);
  m.node_facets_off.assign(1, 0);
  for (int32_t i = 0; i < nnodes; ++i)
  {
    for (int32_t f = 0; f < m.nfacets; ++f)
      if (m.facet_nodes[2 * f] == i || m.facet_nodes[2 * f + 1] == i)
      {
        m.node_facets.push_back(f);
        ++m.node_nfcts[i];
      }
    m.node_facets_off.push_back((int32_t)m.node_facets.size());
  }
  return m;
}

// n x n squares, each cut into four triangles round its centre; corner (i, j) = j (n + 1) + i, centres behind them.
// drop(i, j): the square is left out (its centre node stays in the numbering and belongs to no cell).
template <typename Drop>
Mesh crossed(int n, Drop drop)
{
  std::vector<int32_t> cells;
  const int32_t ncorner = (n + 1) * (n + 1);
  for (int j = 0; j < n; ++j)
    for (int i = 0; i < n; ++i)
    {
      if (drop(i, j))
        continue;
      const int32_t a = j * (n + 1) + i, b = a + 1, c = a + n + 1, d = c + 1, mid = ncorner + j * n + i;
      for (const auto& t : {std::pair<int32_t, int32_t>{a, b}, {b, d}, {d, c}, {c, a}})
      {
        cells.push_back(t.first);
        cells.push_back(t.second);
        cells.push_back(mid);
      }
    }
  return make_mesh(ncorner + n * n, cells);
}

// every one-cell facet primal-Dirichlet, every other facet 0
std::vector<int8_t> valid_types(const Mesh& m, int nrhs)
{
  std::vector<int8_t> ft((size_t)nrhs * m.nfacets, 0);
  for (int r = 0; r < nrhs; ++r)
    for (int32_t f = 0; f < m.nfacets; ++f)
      ft[(size_t)r * m.nfacets + f] = m.boundary(f) ? 1 : 0;
  return ft;
}

std::vector<int32_t> boundary_counts(const Mesh& m)
{
  std::vector<int32_t> b(m.nnodes, -7);
  eqlb::count_node_boundary_facets(m.nnodes, m.node_facets_off.data(), m.node_facets.data(), m.facet_cells_off.data(),
                                   b.data());
  return b;
}

int nfail = 0;

void expect(const char* what, const Mesh& m, int nrhs, const std::vector<int8_t>& ft, const std::vector<uint8_t>* mask,
            int verdict, int32_t index, int32_t row)
{
  const std::vector<int32_t> b = boundary_counts(m);
  const eqlb::TopoFinding tf = eqlb::check_boundary_topology(
      m.nnodes, m.nfacets, nrhs, m.node_ncells.data(), m.node_nfcts.data(), b.data(), m.facet_nodes.data(),
      m.facet_cells_off.data(), ft.data(), mask ? mask->data() : nullptr);
  const bool ok = tf.verdict == verdict && tf.index == index && tf.row == row;
  std::printf("%-58s verdict %d index %3d row %d   expected %d %3d %d   %s\n", what, tf.verdict, (int)tf.index,
              (int)tf.row, verdict, (int)index, (int)row, ok ? "ok" : "WRONG");
  nfail += !ok;
}

void expect_node(const char* what, const Mesh& m, int32_t node, int32_t n, int32_t nf, int32_t b, bool walkable)
{
  const std::vector<int32_t> bc = boundary_counts(m);
  const bool ok = m.node_ncells[node] == n && m.node_nfcts[node] == nf && bc[node] == b
                  && eqlb::node_walkable(m.node_ncells[node], m.node_nfcts[node], bc[node]) == walkable;
  std::printf("%-58s node %2d: %d cells %d facets %d on the boundary, walkable %d   %s\n", what, (int)node,
              (int)m.node_ncells[node], (int)m.node_nfcts[node], (int)bc[node],
              (int)eqlb::node_walkable(m.node_ncells[node], m.node_nfcts[node], bc[node]), ok ? "ok" : "WRONG");
  nfail += !ok;
}
} // namespace

int main()
{
  using eqlb::TOPO_BOUNDARY_FACET_UNTYPED;
  using eqlb::TOPO_INTERIOR_FACET_TYPED;
  using eqlb::TOPO_NODE_NOT_WALKABLE;
  using eqlb::TOPO_OK;

  // --- 2 x 2 crossed square: 9 corners, 4 centres, 16 cells
  const Mesh sq = crossed(2, [](int, int) { return false; });
  expect_node("crossed 2x2: middle corner, closed ring", sq, 4, 8, 8, 0, true);
  expect_node("crossed 2x2: centre of a square, closed ring", sq, 9, 4, 4, 0, true);
  expect_node("crossed 2x2: domain corner, open fan of two cells", sq, 0, 2, 3, 2, true);
  expect_node("crossed 2x2: edge midpoint, open fan of four cells", sq, 1, 4, 5, 2, true);
  expect("crossed 2x2, every boundary facet typed", sq, 1, valid_types(sq, 1), nullptr, TOPO_OK, -1, 0);

  // --- with a hole: the 3 x 3 crossed square without its middle square (a 2 x 2 one has no interior square to drop:
  // every hole in it touches the outer boundary in a node).  The centre node 20 of the dropped square has no cell.
  const Mesh hole = crossed(3, [](int i, int j) { return i == 1 && j == 1; });
  expect_node("hole: corner of the hole, open fan of 6 cells", hole, 5, 6, 7, 2, true);
  expect_node("hole: node without a cell", hole, 20, 0, 0, 0, true);
  expect("hole, both loops typed", hole, 1, valid_types(hole, 1), nullptr, TOPO_OK, -1, 0);
  {
    // the whole inner loop left untyped (a caller that knows the outer boundary only): the first of its facets
    std::vector<int8_t> ft = valid_types(hole, 1);
    const int32_t loop[4] = {hole.facet(5, 6), hole.facet(6, 10), hole.facet(10, 9), hole.facet(9, 5)};
    for (int32_t f : loop)
      ft[f] = 0;
    expect("hole, inner loop untyped", hole, 1, ft, nullptr, TOPO_BOUNDARY_FACET_UNTYPED,
           *std::min_element(loop, loop + 4), 0);
    // ... and accepted where the four corners of the hole are not equilibrated
    std::vector<uint8_t> mask(hole.nnodes, 1);
    for (int32_t nd : {5, 6, 9, 10, 20})
      mask[nd] = 0;
    expect("hole, inner loop untyped, its nodes masked out", hole, 1, ft, &mask, TOPO_OK, -1, 0);
  }

  // --- bow-tie: two pairs of triangles that meet in node 3 only
  const Mesh bow = make_mesh(7, {3, 0, 1, 3, 1, 2, 3, 4, 5, 3, 5, 6});
  expect_node("bow-tie: pinched node, two open fans", bow, 3, 4, 6, 4, false);
  expect("bow-tie", bow, 1, valid_types(bow, 1), nullptr, TOPO_NODE_NOT_WALKABLE, 3, 0);
  {
    std::vector<uint8_t> mask(bow.nnodes, 1);
    mask[3] = 0;
    expect("bow-tie, pinched node masked out", bow, 1, valid_types(bow, 1), &mask, TOPO_OK, -1, 0);
    std::vector<uint8_t> other(bow.nnodes, 1);
    other[0] = 0;
    expect("bow-tie, another node masked out", bow, 1, valid_types(bow, 1), &other, TOPO_NODE_NOT_WALKABLE, 3, 0);
  }

  // --- a node with one cell is an open fan (its patch is refused as too small, which is another check)
  const Mesh two = make_mesh(4, {0, 1, 2, 1, 3, 2});
  expect_node("two triangles: node of one cell", two, 0, 1, 2, 2, true);
  expect("two triangles", two, 1, valid_types(two, 1), nullptr, TOPO_OK, -1, 0);

  // --- one boundary facet of the 2 x 2 square left untyped: row 0, row 1 of two rows
  {
    const int32_t f = sq.facet(1, 2); // bottom edge, right half
    std::vector<int8_t> ft = valid_types(sq, 1);
    ft[f] = 0;
    expect("untyped boundary facet", sq, 1, ft, nullptr, TOPO_BOUNDARY_FACET_UNTYPED, f, 0);
    std::vector<int8_t> ft2 = valid_types(sq, 2);
    ft2[(size_t)sq.nfacets + f] = 0;
    expect("untyped boundary facet on the second row", sq, 2, ft2, nullptr, TOPO_BOUNDARY_FACET_UNTYPED, f, 1);
    std::vector<uint8_t> mask(sq.nnodes, 1);
    mask[1] = 0;
    expect("untyped boundary facet, one of its nodes masked out", sq, 1, ft, &mask, TOPO_BOUNDARY_FACET_UNTYPED, f, 0);
    mask[2] = 0;
    expect("untyped boundary facet, both nodes masked out", sq, 1, ft, &mask, TOPO_OK, -1, 0);
    ft[f] = 2;
    expect("the same facet as a flux-BC facet", sq, 1, ft, nullptr, TOPO_OK, -1, 0);
  }

  // --- a facet between two cells given a type: at a boundary node it could be taken for the start of the walk
  {
    const int32_t f = sq.facet(1, 4); // from the bottom edge to the middle corner
    std::vector<int8_t> ft = valid_types(sq, 1);
    ft[f] = 1;
    expect("typed interior facet", sq, 1, ft, nullptr, TOPO_INTERIOR_FACET_TYPED, f, 0);
    std::vector<int8_t> ft2 = valid_types(sq, 2);
    ft2[(size_t)sq.nfacets + f] = 2;
    expect("typed interior facet on the second row", sq, 2, ft2, nullptr, TOPO_INTERIOR_FACET_TYPED, f, 1);
    std::vector<uint8_t> mask(sq.nnodes, 1);
    mask[4] = 0;
    expect("typed interior facet, one of its nodes masked out", sq, 1, ft, &mask, TOPO_INTERIOR_FACET_TYPED, f, 0);
    mask[1] = 0;
    expect("typed interior facet, both nodes masked out", sq, 1, ft, &mask, TOPO_OK, -1, 0);
  }

  // --- order of the findings: a node before any facet
  {
    std::vector<int8_t> ft = valid_types(bow, 1);
    ft[bow.facet(0, 1)] = 0;
    expect("bow-tie with an untyped facet: the node comes first", bow, 1, ft, nullptr, TOPO_NODE_NOT_WALKABLE, 3, 0);
  }

  if (nfail)
  {
    std::printf("%d verdicts wrong\nFAIL\n", nfail);
    return 1;
  }
  std::printf("PASS\n");
  return 0;
}
