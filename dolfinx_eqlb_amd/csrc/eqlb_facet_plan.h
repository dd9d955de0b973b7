// The table of a facet term of a P_p solver handle (the Robin term of eqlb_primal_set_robin, the spring term of
// eqlb_elasticity_set_springs), built on the host from what the prepare kernel leaves per listed facet
// (eqlb_primal_solve.hip: facet_term_plan).  Plain C++ with no device call, so that a stand-alone program can run it
// under a sanitizer (tools/facet_plan_check.cpp, built and run by tests/test_facet_plan_host.py).
//
// THE RULE.  A listed facet whose flag is 1 (a boundary facet) contributes one entry (row, facet, position, local index)
// for each of its n1 = p + 1 rows; a facet with another flag was skipped and contributes nothing.  The entries are
// sorted by row, then facet id, then list position:
//   rows   [m]      the distinct rows, ascending
//   off    [m + 1]  the entries of rows[k] are ent[off[k]] ... ent[off[k + 1] - 1], so facet ids ascend inside a row
//   ent             list position * 8 + local index
//   chunk  [nch + 1], nch = ceil(ndofs / chunk_dofs): chunk[c] is the first k with rows[k] >= c * chunk_dofs, and
//                   chunk[nch] = m - the piece of rows[] that a chunk of the sum pass searches
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace eqlb
{
// row stride of the rows of a listed facet: the p + 1 <= FACET_ROW rows in the facet's local order, the rest -1
constexpr int FACET_ROW = 5;
// ent packs the local index into three bits; with fewer than FACET_LIST_END listed facets (check_facet_list refuses
// more) position * 8 + local index fits an int32.  The two belong together and are stated here only
constexpr int32_t FACET_LIST_END = 1 << 28;
static_assert(FACET_ROW <= 8, "ent holds list position * 8 + local index");
static_assert((int64_t)(FACET_LIST_END - 1) * 8 + 7 <= INT32_MAX, "ent is an int32");

// where the pieces of a handle's facet table lie in its one array: facets [n] | dofs [n][FACET_ROW] | chunk | rows [m] |
// off [m + 1] | ent, from the piece sizes
struct FacetLayout
{
  size_t dofs = 0, chunk = 0, rows = 0, off = 0, ent = 0, total = 0;
  FacetLayout() = default;
  FacetLayout(size_t n, size_t nchunk, size_t m, size_t nent)
      : dofs(n), chunk(n * (1 + FACET_ROW)), rows(chunk + nchunk), off(rows + m), ent(off + m + 1), total(ent + nent)
  {
  }
  size_t m() const { return off - rows; }
};

struct FacetTable
{
  std::vector<int32_t> rows, off, ent, chunk;
  FacetLayout at;
};

// flag [n], facet [n] and dofs [n][FACET_ROW] per listed facet (of dofs the first n1 count); chunk_dofs: the DOFs of a
// chunk of the sum pass
inline FacetTable facet_plan(size_t n, const int32_t* flag, const int32_t* facet, const int32_t* dofs, int n1,
                             int64_t ndofs, int chunk_dofs)
{
  struct Entry
  {
    int32_t row, facet, pos, loc;
  };
  std::vector<Entry> ent;
  for (size_t i = 0; i < n; ++i)
  {
    if (flag[i] != 1)
      continue; // (device memory space: skipped)
    for (int j = 0; j < n1; ++j)
      ent.push_back(Entry{dofs[i * FACET_ROW + j], facet[i], (int32_t)i, j});
  }
  std::sort(ent.begin(), ent.end(), [](const Entry& a, const Entry& b) {
    return a.row != b.row ? a.row < b.row : a.facet != b.facet ? a.facet < b.facet : a.pos < b.pos;
  });
  FacetTable t;
  t.ent.resize(ent.size());
  for (size_t k = 0; k < ent.size(); ++k)
  {
    if (k == 0 || ent[k].row != ent[k - 1].row)
    {
      t.rows.push_back(ent[k].row);
      t.off.push_back((int32_t)k);
    }
    t.ent[k] = ent[k].pos * 8 + ent[k].loc;
  }
  t.off.push_back((int32_t)ent.size());
  const size_t nch = (size_t)((ndofs + chunk_dofs - 1) / chunk_dofs);
  t.chunk.resize(nch + 1);
  for (size_t c = 0; c <= nch; ++c)
    t.chunk[c] = (int32_t)(std::lower_bound(t.rows.begin(), t.rows.end(),
                                            (int32_t)std::min<int64_t>((int64_t)c * chunk_dofs, INT32_MAX))
                           - t.rows.begin());
  t.chunk[nch] = (int32_t)t.rows.size();
  t.at = FacetLayout(n, t.chunk.size(), t.rows.size(), t.ent.size());
  return t;
}
} // namespace eqlb
