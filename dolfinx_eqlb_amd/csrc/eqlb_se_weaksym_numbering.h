// The integer rules of the weak-symmetry step, once for its three kernels (eqlb_se_weaksym_common.h says what they
// share): which unknowns and multipliers a patch has, where the local unknowns [d | um | up | ua] of cell i of the fan
// sit in the dense numbering (k_se_weaksym) and in the chain + border numbering (k_se_weaksym_banded, _large), which
// multiplier belongs to a local vertex, and which unknowns a flux BC fixes.  Plain C++ with no device call, so that a
// stand-alone program checks it on the host (tools/weaksym_numbering_check.cpp, built and run by
// tests/test_weaksym_numbering_host.py).
#pragma once

#if defined(__HIPCC__)
#define EQLB_WS_FN __host__ __device__ __forceinline__
#define EQLB_WS_UNROLL _Pragma("unroll")
#else
#define EQLB_WS_FN inline
#define EQLB_WS_UNROLL
#endif

namespace eqlb
{

// A vertex patch of n cells T_1 ... T_n around its node: facets 0 ... nf - 1 (facet i lies before cell i; an interior
// patch is a ring, its last cell ends on facet 0; a boundary patch is a fan that ends on facet n), points 0 (the node)
// and 1 ... nf (the ring), and the flux BCs of the two stress rows on the first / last facet of a fan
// (PatchData::reinitialisation :175-206).
struct WsPatch
{
  // (scalars, not arrays: a member indexed by a loop variable keeps the whole record in memory until the loop is
  // unrolled, and the kernels lose the early passes of the compiler over it)
  bool interior;
  int n, nf, npnt;
  bool bc0_row0, bc0_row1, bcn_row0, bcn_row1, requires_bcs;
  bool meanvalue; // mean-value multiplier unless some row has a primal-Dirichlet end (type essnt_primal or mixed)
  int dim_c;      // multipliers: the points (+ the mean value)

  EQLB_WS_FN WsPatch(bool interior_, int n_, bool bc0_0, bool bcn_0, bool bc0_1, bool bcn_1)
      : interior(interior_), n(n_), nf(interior_ ? n_ : n_ + 1), npnt(nf + 1), bc0_row0(bc0_0), bc0_row1(bc0_1),
        bcn_row0(bcn_0), bcn_row1(bcn_1), requires_bcs(bc0_0 || bcn_0 || bc0_1 || bcn_1),
        meanvalue(interior_ || (bc0_0 && bcn_0 && bc0_1 && bcn_1)), dim_c(meanvalue ? npnt + 1 : npnt)
  {
  }
  // flux BC of stress row k on the first / the last facet of the fan
  EQLB_WS_FN bool bc0(int k) const { return k ? bc0_row1 : bc0_row0; }
  EQLB_WS_FN bool bcn(int k) const { return k ? bcn_row1 : bcn_row0; }
  // the facet behind cell i
  EQLB_WS_FN int next_facet(int i) const { return interior ? ((i + 1 < n) ? i + 1 : 0) : i + 1; }
};

// multiplier DOF (point) of the local vertices of cell i with local facets fm, fp and node ln (se/Patch.hpp:621-708)
EQLB_WS_FN void ws_points(const WsPatch& p, int i, int fm, int fp, int ln, int pj[3])
{
  const int v_ea = 3 - fp - ln, v_eam1 = 3 - fm - ln;
  const int p_ea = p.interior ? i + 1 : ((i + 1 == p.n) ? p.nf : i + 1);
  const int p_eam1 = p.interior ? ((i == 0) ? p.n : i) : ((i == 0) ? p.nf - 1 : i);
  EQLB_WS_UNROLL
  for (int j = 0; j < 3; ++j)
    pj[j] = (j == ln) ? 0 : ((j == v_ea) ? p_ea : ((j == v_eam1) ? p_eam1 : 0));
}

// H(div=0) unknowns of RT_K: per facet KB, per cell NADD bubbles, one of the node; a cell sees NH of them
template <int K>
struct WsNumbering
{
  static constexpr int KB = K - 1, NADD = (K - 1) * (K - 2) / 2, NH = 1 + 2 * KB + NADD;
  static EQLB_WS_FN int dim(const WsPatch& p) { return 1 + KB * p.nf + NADD * p.n; }
  // dense numbering [d | x_0 ... x_{nf-1} | a_0 ... a_{n-1}]
  static EQLB_WS_FN void gi(const WsPatch& p, int i, int out[NH])
  {
    const int fi_p = p.next_facet(i);
    out[0] = 0;
    EQLB_WS_UNROLL
    for (int j = 0; j < KB; ++j)
    {
      out[1 + j] = 1 + i * KB + j;
      out[1 + KB + j] = 1 + fi_p * KB + j;
    }
    EQLB_WS_UNROLL
    for (int q = 0; q < NADD; ++q)
      out[1 + 2 * KB + q] = 1 + p.nf * KB + i * NADD + q;
  }
  // fixed (flux-BC) unknowns per row k (se/assembly.hpp:46-98): local unknown h of cell i
  static EQLB_WS_FN bool fixed(const WsPatch& p, int k, int h, int i)
  {
    if (!p.requires_bcs)
      return false;
    if (h == 0)
      return p.bc0(k) || p.bcn(k);
    if (h <= KB)
      return p.bc0(k) && i == 0;
    if (h <= 2 * KB)
      return p.bcn(k) && i == p.n - 1;
    return false;
  }
};

// The unknowns ordered as a banded chain plus a border:
//   chain   [a_0 | x_1 | a_1 | x_2 | ... ]   a_s: the NADD bubbles of cell s, x_f: the KB unknowns of facet f >= 1
//   border  [d | x_0]                        the node unknown and facet 0 (closes the ring of interior patches)
// A cell couples [x_s | a_s | x_{s+1}] and the border only: half bandwidth BW, rows of LDB entries.
template <int K>
struct WsChain : WsNumbering<K>
{
  using WsNumbering<K>::KB;
  using WsNumbering<K>::NADD;
  using WsNumbering<K>::NH;
  static constexpr int NBD = 1 + KB;           // border: d, x_0
  static constexpr int BW = 2 * KB + NADD - 1; // half bandwidth of the chain
  static constexpr int LDB = BW + 1;
  static EQLB_WS_FN int nch(const WsPatch& p) { return WsNumbering<K>::dim(p) - NBD; }
  static EQLB_WS_FN int pos_facet(int nch, int f, int m)
  {
    return (f == 0) ? nch + 1 + m : (f - 1) * (KB + NADD) + NADD + m;
  }
  static EQLB_WS_FN void pos(const WsPatch& p, int i, int out[NH])
  {
    const int nc = nch(p), fi_p = p.next_facet(i);
    out[0] = nc;
    EQLB_WS_UNROLL
    for (int j = 0; j < KB; ++j)
    {
      out[1 + j] = pos_facet(nc, i, j);
      out[1 + KB + j] = pos_facet(nc, fi_p, j);
    }
    EQLB_WS_UNROLL
    for (int q = 0; q < NADD; ++q)
      out[1 + 2 * KB + q] = i * (KB + NADD) + q;
  }
  // slot of vertex j in the compressed row of B of local unknown h >= 1: 0 the patch node, 1 the ring point of the
  // row's facet (of facet s for the bubbles of cell s), 2 / 3 the other ring point of the cell before / after it
  static EQLB_WS_FN int bslot(int fm, int fp, int ln, int h, int j)
  {
    if (j == ln)
      return 0;
    const int v_ea = 3 - fp - ln, v_eam1 = 3 - fm - ln;
    const bool uprow = h > KB && h <= 2 * KB;
    return uprow ? ((j == v_ea) ? 1 : 2) : ((j == v_eam1) ? 1 : 3);
  }
};

} // namespace eqlb
