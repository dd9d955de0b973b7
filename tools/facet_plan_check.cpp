// The table of a facet term (dolfinx_eqlb_amd/csrc/eqlb_facet_plan.h), printed for a few hand-written lists by a program
// of its own: the header is all it includes of the library, so it builds with any host compiler and runs under the
// sanitizers (tests/test_facet_plan_host.py holds the lines this prints).
#include "../dolfinx_eqlb_amd/csrc/eqlb_facet_plan.h"

#include <cstdio>
#include <vector>

using namespace eqlb;

// a listed facet as the prepare kernel leaves it: the flag, the id and the rows in the facet's local order
struct Listed
{
  int32_t flag, facet;
  int32_t dofs[FACET_ROW];
};
constexpr int32_t X = -1; // no row

static void line(const char* name, const std::vector<int32_t>& v)
{
  printf("%s:", name);
  for (int32_t x : v)
    printf(" %d", (int)x);
  printf("\n");
}

static void show(const char* name, const std::vector<Listed>& list, int n1, int64_t ndofs, int chunk_dofs)
{
  std::vector<int32_t> flag, facet, dofs;
  for (const Listed& f : list)
  {
    flag.push_back(f.flag);
    facet.push_back(f.facet);
    dofs.insert(dofs.end(), f.dofs, f.dofs + FACET_ROW);
  }
  const FacetTable t = facet_plan(list.size(), flag.data(), facet.data(), dofs.data(), n1, ndofs, chunk_dofs);
  printf("case %s\n", name);
  line("rows", t.rows);
  line("off", t.off);
  line("ent", t.ent);
  line("chunk", t.chunk);
  printf("layout: %zu %zu %zu %zu %zu %zu, m %zu\n", t.at.dofs, t.at.chunk, t.at.rows, t.at.off, t.at.ent, t.at.total,
         t.at.m());
}

int main()
{
  // two triangles on the nodes 0 ... 3, the diagonal is facet 2: the boundary facets 0 (0, 1), 1 (0, 2), 3 (1, 3),
  // 4 (2, 3); the facet rows of p = 3 are 4 + 2 f + j
  show("pair p=1", {{1, 0, {0, 1, X, X, X}}, {1, 1, {0, 2, X, X, X}}, {1, 3, {1, 3, X, X, X}}, {1, 4, {2, 3, X, X, X}}}, 2,
       4, 256);
  show("pair p=3",
       {{1, 0, {0, 1, 4, 5, X}}, {1, 1, {0, 2, 6, 7, X}}, {1, 3, {1, 3, 10, 11, X}}, {1, 4, {2, 3, 12, 13, X}}}, 4, 16,
       128);
  // the pinch node 0 of a bowtie lies in the four listed facets 0 ... 3 = (0, 1) ... (0, 4); then the list backwards
  show("pinch", {{1, 0, {0, 1, X, X, X}}, {1, 1, {0, 2, X, X, X}}, {1, 2, {0, 3, X, X, X}}, {1, 3, {0, 4, X, X, X}}}, 2, 5,
       256);
  show("descending", {{1, 3, {0, 4, X, X, X}}, {1, 2, {0, 3, X, X, X}}, {1, 1, {0, 2, X, X, X}}, {1, 0, {0, 1, X, X, X}}},
       2, 5, 256);
  // p = 2 on 6 nodes (facet row 6 + f): skipped positions in front, in the middle and at the end
  show("skipped",
       {{0, 99, {X, X, X, X, X}},
        {1, 2, {1, 4, 8, X, X}},
        {2, 5, {X, X, X, X, X}},
        {1, 7, {4, 5, 13, X, X}},
        {0, -3, {X, X, X, X, X}}},
       3, 20, 256);
  // rows on both sides of a chunk boundary; ndofs a multiple of the chunk and one more
  const std::vector<Listed> edge{{1, 10, {100, 255, X, X, X}}, {1, 11, {255, 256, X, X, X}}, {1, 12, {256, 511, X, X, X}}};
  std::vector<Listed> over = edge;
  over.push_back({1, 13, {511, 512, X, X, X}});
  show("512 by 256", edge, 2, 512, 256);
  show("512 by 128", edge, 2, 512, 128);
  show("513 by 256", over, 2, 513, 256);
  show("513 by 128", over, 2, 513, 128);
  show("nothing left", {{0, 7, {X, X, X, X, X}}, {2, 2, {X, X, X, X, X}}}, 2, 4, 256);
  return 0;
}
