// Stand-alone check of the integer rules of the weak-symmetry kernels
// (dolfinx_eqlb_amd/csrc/eqlb_se_weaksym_numbering.h): the dense numbering gi, the chain + border numbering pos, the
// points pj of the multipliers, the slots of a compressed row of B and the unknowns a flux BC fixes.  For K = 2, 3, 4,
// interior and boundary patches, n = 2 ... 64 cells (the chain also n = 65, 200, 1000) and every combination of the
// flux-BC flags of the two stress rows.  Built by tests/test_weaksym_numbering_host.py with
// -fsanitize=address,undefined where the compiler has the runtimes.  Prints the number of patches checked; the first
// rule that fails is printed and ends the program with status 1.
#include "../dolfinx_eqlb_amd/csrc/eqlb_se_weaksym_numbering.h"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

using namespace eqlb;

namespace
{
long checked = 0;
const char* numbering_name = "";
int K_now = 0;

[[noreturn]] void fail(const char* rule, const WsPatch& p, int i)
{
  std::printf("FAILED %s: K %d %s interior %d n %d cell %d bc0 %d%d bcn %d%d\n", rule, K_now, numbering_name,
              p.interior ? 1 : 0, p.n, i, p.bc0(0) ? 1 : 0, p.bc0(1) ? 1 : 0, p.bcn(0) ? 1 : 0, p.bcn(1) ? 1 : 0);
  std::exit(1);
}
#define REQUIRE(cond, rule, p, i) \
  do \
  { \
    if (!(cond)) \
      fail(rule, p, i); \
  } while (0)

// the local facets and the node of cell i: every ordered choice of three distinct local ids occurs
void local_ids(int i, int& fm, int& fp, int& ln)
{
  static const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  fm = perm[i % 6][0];
  fp = perm[i % 6][1];
  ln = perm[i % 6][2];
}

// what holds for a numbering num(cell) -> NH positions, whichever of the two it is
template <int K, class Num>
void check_numbering(const WsPatch& p, Num num, std::vector<std::vector<int>>& where)
{
  using N = WsNumbering<K>;
  constexpr int KB = N::KB, NH = N::NH;
  const int dim = N::dim(p);
  where.assign(p.n, std::vector<int>(NH));
  std::vector<int> hits(dim, 0);
  for (int i = 0; i < p.n; ++i)
  {
    int out[NH];
    num(i, out);
    std::set<int> own;
    for (int h = 0; h < NH; ++h)
    {
      REQUIRE(out[h] >= 0 && out[h] < dim, "a position lies in 0 ... dim - 1", p, i);
      REQUIRE(own.insert(out[h]).second, "the unknowns of a cell are distinct", p, i);
      ++hits[out[h]];
      where[i][h] = out[h];
    }
  }
  // the union is exactly 0 ... dim - 1: d in every cell, a facet in its two cells (the ends of a fan in one), a bubble
  // in one
  for (int q = 0; q < dim; ++q)
    REQUIRE(hits[q] >= 1, "every unknown belongs to a cell", p, q);
  for (int i = 0; i < p.n; ++i)
  {
    REQUIRE(where[i][0] == where[0][0], "all cells share d", p, i);
    const bool last = i + 1 == p.n;
    if (last && !p.interior)
      break;
    const int nb = last ? 0 : i + 1; // the ring closes on facet 0
    for (int j = 0; j < KB; ++j)
      REQUIRE(where[i][1 + KB + j] == where[nb][1 + j], "neighbours agree on the facet they share", p, i);
  }
  // fixed marks d, the unknowns of facet 0 and of the last facet (in a ring that is facet 0 again), per row's flags
  for (int k = 0; k < 2; ++k)
  {
    std::set<int> marked, expected;
    for (int i = 0; i < p.n; ++i)
      for (int h = 0; h < NH; ++h)
        if (N::fixed(p, k, h, i))
          marked.insert(where[i][h]);
    if (p.bc0(k) || p.bcn(k))
      expected.insert(where[0][0]);
    for (int j = 0; j < KB; ++j)
    {
      if (p.bc0(k))
        expected.insert(where[0][1 + j]);
      if (p.bcn(k))
        expected.insert(where[p.n - 1][1 + KB + j]);
    }
    REQUIRE(marked == expected, "fixed marks d, facet 0 and the last facet by the row's flags", p, k);
    // (the set-up gives the flags to fans only, eqlb_patch_builder.hip; in a ring the first and the last cell would
    // have to agree on facet 0, which the rule does not ask of them)
    for (int i = 0; i < p.n && !p.interior; ++i)
      for (int h = 0; h < NH; ++h)
        REQUIRE(N::fixed(p, k, h, i) == (expected.count(where[i][h]) != 0),
                "every cell of a fixed unknown sees it fixed", p, i);
  }
}

template <int K>
void check_patch(const WsPatch& p, bool dense)
{
  using N = WsNumbering<K>;
  using C = WsChain<K>;
  constexpr int KB = N::KB, NADD = N::NADD, NH = N::NH;
  K_now = K;
  static_assert(NH == 1 + 2 * KB + NADD && C::NBD == 1 + KB && C::BW == 2 * KB + NADD - 1 && C::LDB == C::BW + 1, "");
  REQUIRE(p.nf == (p.interior ? p.n : p.n + 1) && p.npnt == p.nf + 1, "facets and points", p, 0);
  REQUIRE(N::dim(p) == 1 + KB * p.nf + NADD * p.n, "unknowns", p, 0);
  const bool dual = !p.interior && p.bc0(0) && p.bcn(0) && p.bc0(1) && p.bcn(1);
  REQUIRE(p.meanvalue == (p.interior || dual) && p.dim_c == p.npnt + (p.meanvalue ? 1 : 0), "mean-value rule", p, 0);
  REQUIRE(p.requires_bcs == (p.bc0(0) || p.bc0(1) || p.bcn(0) || p.bcn(1)), "requires_bcs", p, 0);

  std::vector<std::vector<int>> where;
  if (dense)
  {
    numbering_name = "gi";
    check_numbering<K>(p, [&](int i, int* out) { N::gi(p, i, out); }, where);
  }
  numbering_name = "pos";
  check_numbering<K>(p, [&](int i, int* out) { C::pos(p, i, out); }, where);
  const int nch = C::nch(p);
  REQUIRE(nch == N::dim(p) - C::NBD && where[0][0] == nch, "the border starts with d", p, 0);
  for (int m = 0; m < KB; ++m)
    REQUIRE(C::pos_facet(nch, 0, m) == nch + 1 + m && where[0][1 + m] == nch + 1 + m, "facet 0 lies in the border", p, 0);
  if (!p.interior)
    for (int m = 0; m < KB; ++m)
      REQUIRE(C::pos_facet(nch, p.n, m) == where[p.n - 1][1 + KB + m], "pos_facet(n) is the last facet of a fan", p, 0);
  for (int i = 0; i < p.n; ++i)
    for (int h = 0; h < NH; ++h)
      for (int g = 0; g < NH; ++g)
      {
        const int a = where[i][h], b = where[i][g];
        REQUIRE(a >= nch || b >= nch || std::abs(a - b) <= C::BW, "a chain entry lies within the half bandwidth", p, i);
      }

  numbering_name = "pj";
  int prev_ea = -1, first_eam1 = -1;
  for (int i = 0; i < p.n; ++i)
  {
    int fm, fp, ln, pj[3];
    local_ids(i, fm, fp, ln);
    ws_points(p, i, fm, fp, ln, pj);
    const int v_ea = 3 - fp - ln, v_eam1 = 3 - fm - ln;
    for (int j = 0; j < 3; ++j)
      REQUIRE(pj[j] >= 0 && pj[j] < p.npnt, "a point lies in 0 ... npnt - 1", p, i);
    REQUIRE(pj[ln] == 0 && pj[v_ea] != 0 && pj[v_eam1] != 0 && pj[v_ea] != pj[v_eam1],
            "the node is point 0, the ring points are two others", p, i);
    if (i > 0)
      REQUIRE(pj[v_eam1] == prev_ea, "consecutive cells share the ring point between them", p, i);
    else
      first_eam1 = pj[v_eam1];
    prev_ea = pj[v_ea];
    for (int h = 1; h < NH; ++h)
    {
      std::set<int> slots;
      for (int j = 0; j < 3; ++j)
      {
        const int s = C::bslot(fm, fp, ln, h, j);
        REQUIRE(s >= 0 && s <= 3 && (s == 0) == (j == ln), "bslot is 0 ... 3, and 0 exactly for the node", p, i);
        REQUIRE(slots.insert(s).second, "the vertices of a cell take different slots of a row", p, i);
      }
    }
  }
  REQUIRE(p.interior ? prev_ea == first_eam1 : prev_ea != first_eam1, "the ring of points closes, a fan does not", p, 0);
  {
    // the points of all cells are exactly 0 ... npnt - 1
    std::set<int> pts;
    for (int i = 0; i < p.n; ++i)
    {
      int fm, fp, ln, pj[3];
      local_ids(i, fm, fp, ln);
      ws_points(p, i, fm, fp, ln, pj);
      pts.insert(pj, pj + 3);
    }
    REQUIRE((int)pts.size() == p.npnt, "every point belongs to a cell", p, 0);
  }
  ++checked;
}

template <int K>
void check_degree()
{
  std::vector<int> sizes;
  for (int n = 2; n <= 64; ++n)
    sizes.push_back(n);
  for (int n : {65, 200, 1000})
    sizes.push_back(n);
  for (int n : sizes)
    for (int interior = 0; interior < 2; ++interior)
      for (int flags = 0; flags < 16; ++flags)
      {
        const WsPatch p(interior != 0, n, (flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0, (flags & 8) != 0);
        check_patch<K>(p, n <= 64);
      }
}
} // namespace

int main()
{
  check_degree<2>();
  check_degree<3>();
  check_degree<4>();
  std::printf("checked %ld patches\n", checked);
  return 0;
}
