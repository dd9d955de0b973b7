// Host emulation of the lane arithmetic of the RT_2 full-patch body (dolfinx_eqlb_amd/csrc/eqlb_pair_chain.h):
// the pair-lane mapping (4 lanes, two ring cells each) and the lane = cell mapping (8 lanes) run from the same
// templates with the lanes of a patch emulated as array indices, on the same random rings of 8 cells, and are compared
// with each other and with a dense solve / a sequential walk round the ring.
//
//   c++ -O1 -g -std=c++17 [-fsanitize=address,undefined] tools/pair_chain_emul.cpp -o pair_chain_emul && ./pair_chain_emul
//
// exit status 0: every ring within the bounds (printed).  No GPU, no HIP.
//
//   ./pair_chain_emul degenerate [draws]
//
// rings with one cell of det J = 0, their te / le blocks built as phase C builds them (metric J^T J / |det J| times
// reference tensors: inf and NaN entries), the bad cell on each of the eight ring positions; and a healthy ring with a
// single +inf that reaches the last pivot only.  exit status 0: `ok` of pair_chain came back false in some lane of every
// such ring (the device raises the status word from any lane) and true in every lane of the healthy rings; cell_chain
// with the pivot test of se_patch_body (a > 0) is held to the same on the flat cells, its count for the lone +inf is
// printed only.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>

#include "../dolfinx_eqlb_amd/csrc/eqlb_pair_chain.h"

namespace
{
template <int N>
struct Vec
{
  double v[N];
};
template <int N>
struct Mask
{
  bool v[N];
};
#define EQLB_VEC_OP(OP)                                                                             \
  template <int N>                                                                                  \
  Vec<N> operator OP(const Vec<N>& a, const Vec<N>& b)                                              \
  {                                                                                                 \
    Vec<N> r;                                                                                       \
    for (int i = 0; i < N; ++i)                                                                     \
      r.v[i] = a.v[i] OP b.v[i];                                                                    \
    return r;                                                                                       \
  }
EQLB_VEC_OP(+)
EQLB_VEC_OP(-)
EQLB_VEC_OP(*)
#undef EQLB_VEC_OP
template <int N>
Vec<N> operator-(const Vec<N>& a)
{
  Vec<N> r;
  for (int i = 0; i < N; ++i)
    r.v[i] = -a.v[i];
  return r;
}

// lanes of ONE patch group as array indices
template <int N>
struct Lanes
{
  using T = Vec<N>;
  using mask = Mask<N>;
  template <class F>
  static T map(F f)
  {
    T r;
    for (int i = 0; i < N; ++i)
      r.v[i] = f(i);
    return r;
  }
  static T cst(double c) { return map([&](int) { return c; }); }
  static T fma(const T& a, const T& b, const T& c) { return map([&](int i) { return std::fma(a.v[i], b.v[i], c.v[i]); }); }
  static T rcp(const T& a) { return map([&](int i) { return 1.0 / a.v[i]; }); }
  // a pivot passes if it is positive AND finite (PairDpp::pos of eqlb_se_kernels_pair.hip: one class test)
  static mask pos(const T& a)
  {
    mask m;
    for (int i = 0; i < N; ++i)
      m.v[i] = a.v[i] > 0.0 && a.v[i] < std::numeric_limits<double>::infinity();
    return m;
  }
  static mask both(const mask& a, const mask& b)
  {
    mask m;
    for (int i = 0; i < N; ++i)
      m.v[i] = a.v[i] && b.v[i];
    return m;
  }
  static T dn(const T& a) { return map([&](int i) { return a.v[(i + N - 1) % N]; }); }
  static T up(const T& a) { return map([&](int i) { return a.v[(i + 1) % N]; }); }
  static T dn2(const T& a) { return map([&](int i) { return a.v[(i + N - 2) % N]; }); }
  static T b0(const T& a) { return map([&](int) { return a.v[0]; }); }
  // butterfly sums in the order of the device code: xor 1, xor 2 (, i <-> N - 1 - i)
  static T qsum(const T& a)
  {
    T s = map([&](int i) { return a.v[i] + a.v[i ^ 1]; });
    return map([&](int i) { return s.v[i] + s.v[i ^ 2]; });
  }
  static T gsum(const T& a)
  {
    const T s = qsum(a);
    return map([&](int i) { return s.v[i] + s.v[N - 1 - i]; });
  }
  static T z0(const T& a) { return map([&](int i) { return i == 0 ? 0.0 : a.v[i]; }); }
  static T z01(const T& a) { return map([&](int i) { return i <= 1 ? 0.0 : a.v[i]; }); }
  static T z3(const T& a) { return map([&](int i) { return i == 3 ? 0.0 : a.v[i]; }); }
  static T zlast(const T& a) { return map([&](int i) { return i == N - 1 ? 0.0 : a.v[i]; }); }
  static T one0(const T& a) { return map([&](int i) { return i == 0 ? 1.0 : a.v[i]; }); }
  static T only0(const T& a) { return map([&](int i) { return i == 0 ? a.v[i] : 0.0; }); }
  static T only1(const T& a) { return map([&](int i) { return i == 1 ? a.v[i] : 0.0; }); }
  static T only3(const T& a) { return map([&](int i) { return i == 3 ? a.v[i] : 0.0; }); }
  static T onlylast(const T& a) { return map([&](int i) { return i == N - 1 ? a.v[i] : 0.0; }); }
  static T sel0(const T& a, const T& b) { return map([&](int i) { return i == 0 ? a.v[i] : b.v[i]; }); }
  static T shr(const T& a, int S) { return map([&](int i) { return i >= S ? a.v[i - S] : 0.0; }); }
  static T shl(const T& a, int S) { return map([&](int i) { return i + S < N ? a.v[i + S] : 0.0; }); }
  static T pre(const T& a, int S) { return shr(a, S); }
};
using Q4 = Lanes<4>;
// the yardstick keeps the pivot test of se_patch_body, a > 0: a lone +inf passes it (reported, not asserted, below)
struct C8 : Lanes<8>
{
  static mask pos(const T& a)
  {
    mask m;
    for (int i = 0; i < 8; ++i)
      m.v[i] = a.v[i] > 0.0;
    return m;
  }
};

// dense reference: 9 unknowns [d | x_0 .. x_7], Gaussian elimination with partial pivoting
void dense_solve(const double te[8][6], const double le[8][3], double d_x[9])
{
  double A[9][10] = {};
  for (int i = 0; i < 8; ++i)
  {
    const int gi[3] = {0, 1 + i, 1 + (i + 1) % 8};
    for (int h = 0; h < 3; ++h)
    {
      A[gi[h]][9] += le[i][h];
      for (int g = 0; g < 3; ++g)
        A[gi[h]][gi[g]] += te[i][(h >= g) ? h * (h + 1) / 2 + g : g * (g + 1) / 2 + h];
    }
  }
  for (int c = 0; c < 9; ++c)
  {
    int p = c;
    for (int r = c + 1; r < 9; ++r)
      if (std::fabs(A[r][c]) > std::fabs(A[p][c]))
        p = r;
    for (int j = 0; j < 10; ++j)
      std::swap(A[c][j], A[p][j]);
    for (int r = c + 1; r < 9; ++r)
    {
      const double f = A[r][c] / A[c][c];
      for (int j = c; j < 10; ++j)
        A[r][j] -= f * A[c][j];
    }
  }
  for (int r = 8; r >= 0; --r)
  {
    double s = A[r][9];
    for (int j = r + 1; j < 9; ++j)
      s -= A[r][j] * d_x[j];
    d_x[r] = s / A[r][r];
  }
}

void rev2_ref(double x0, double x1, bool rev, double& y0, double& y1)
{
  y0 = x0;
  y1 = rev ? x0 - x1 : x1; // B = [[1, 0], [1, -1]]
}

// ---- rings with a degenerate cell ----------------------------------------------------------------------------------
// One cell as phase C of the device code builds it: te = g0 T0 + g1 T1 + g2 T2 and le = -(g0 s0 + g1 s1 + g2 s2) with the
// metric g = J^T J / |det J| (ia = 1 / |det J| is +inf on a flat cell) and reference tensors T_x [6], s_x [3].  The
// tensors are those of three vector fields v_h sampled at NP points: T0 = sum v_h,0 v_g,0, T2 = sum v_h,1 v_g,1,
// T1 = sum (v_h,0 v_g,1 + v_h,1 v_g,0) - with an SPD metric te is the Gram matrix of the fields, i.e. SPD.
struct RefCell
{
  static constexpr int NP = 4;
  double v[3][NP][2], s[3][3];
  double T[3][6];
  void tensors()
  {
    for (int h = 0; h < 3; ++h)
      for (int g = 0; g <= h; ++g)
      {
        double t0 = 0.0, t1 = 0.0, t2 = 0.0;
        for (int q = 0; q < NP; ++q)
        {
          t0 += v[h][q][0] * v[g][q][0];
          t1 += v[h][q][0] * v[g][q][1] + v[h][q][1] * v[g][q][0];
          t2 += v[h][q][1] * v[g][q][1];
        }
        T[0][h * (h + 1) / 2 + g] = t0;
        T[1][h * (h + 1) / 2 + g] = t1;
        T[2][h * (h + 1) / 2 + g] = t2;
      }
  }
  void build(const double J[4], double te[6], double le[3]) const
  {
    const double J00 = J[0], J01 = J[1], J10 = J[2], J11 = J[3];
    const double detJ = J00 * J11 - J01 * J10;
    const double ia = 1.0 / std::fabs(detJ);
    const double g0 = (J00 * J00 + J10 * J10) * ia, g1 = (J00 * J01 + J10 * J11) * ia, g2 = (J01 * J01 + J11 * J11) * ia;
    for (int e = 0; e < 6; ++e)
      te[e] = g0 * T[0][e] + g1 * T[1][e] + g2 * T[2][e];
    for (int h = 0; h < 3; ++h)
      le[h] = -(g0 * s[0][h] + g1 * s[1][h] + g2 * s[2][h]);
  }
};

// `ok` of both mappings on one ring: (every lane true, some lane false) per mapping
struct Flags
{
  bool pair_all, pair_any_false, cell_all, cell_any_false;
};
Flags run_chains(const double te[8][6], const double le[8][3])
{
  Flags fl{true, false, true, false};
  {
    C8::T t[6], l[3], d, xm, xp;
    C8::mask ok;
    for (int e = 0; e < 6; ++e)
      t[e] = C8::map([&](int i) { return te[i][e]; });
    for (int h = 0; h < 3; ++h)
      l[h] = C8::map([&](int i) { return le[i][h]; });
    eqlb_pair::cell_chain<C8::T, C8>(t, l, d, xm, xp, ok);
    for (int i = 0; i < 8; ++i)
    {
      fl.cell_all = fl.cell_all && ok.v[i];
      fl.cell_any_false = fl.cell_any_false || !ok.v[i];
    }
  }
  {
    Q4::T t[2][6], l[2][3], d, xe, xo, xn;
    Q4::mask ok;
    for (int c = 0; c < 2; ++c)
    {
      for (int e = 0; e < 6; ++e)
        t[c][e] = Q4::map([&](int i) { return te[2 * i + c][e]; });
      for (int h = 0; h < 3; ++h)
        l[c][h] = Q4::map([&](int i) { return le[2 * i + c][h]; });
    }
    eqlb_pair::pair_chain<Q4::T, Q4>(t, l, d, xe, xo, xn, ok);
    for (int i = 0; i < 4; ++i)
    {
      fl.pair_all = fl.pair_all && ok.v[i];
      fl.pair_any_false = fl.pair_any_false || !ok.v[i];
    }
  }
  return fl;
}

int degenerate_rings(int ndraw)
{
  std::mt19937_64 rng(20261021);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  const double inf = std::numeric_limits<double>::infinity();
  int healthy_flagged = 0, missed_pair = 0, missed_cell = 0, nbad = 0, with_nan = 0, with_inf = 0;
  int inf_missed_pair = 0, inf_missed_cell = 0, ninf = 0;
  for (int it = 0; it < ndraw; ++it)
  {
    // axis: every sample of every field along x or along y - T1 = 0, so an infinite g1 meets exact zeros
    const bool axis = it % 4 == 3;
    RefCell ref[8];
    double J[8][4], te[8][6], le[8][3];
    for (int i = 0; i < 8; ++i)
    {
      for (int h = 0; h < 3; ++h)
      {
        for (int q = 0; q < RefCell::NP; ++q)
        {
          ref[i].v[h][q][0] = U(rng);
          ref[i].v[h][q][1] = U(rng);
          if (axis)
            ref[i].v[h][q][(q + h) & 1] = 0.0;
        }
        for (int x = 0; x < 3; ++x)
          ref[i].s[x][h] = U(rng);
      }
      ref[i].tensors();
      // a cell of positive or negative orientation, |det J| between 1/4 and 4
      do
      {
        for (double& v : J[i])
          v = 2.0 * U(rng);
      } while (std::fabs(J[i][0] * J[i][3] - J[i][1] * J[i][2]) < 0.25);
      ref[i].build(J[i], te[i], le[i]);
    }
    const Flags h = run_chains(te, le);
    if (!h.pair_all || !h.cell_all)
      ++healthy_flagged;
    // the bad cell: dyadic columns, so det J is exactly zero - parallel columns, a zero column, a zero row
    for (int kind = 0; kind < 4; ++kind)
      for (int pos = 0; pos < 8; ++pos)
      {
        const double a = std::ldexp(1.0 + (double)(rng() % 7), -3), b = std::ldexp(1.0 + (double)(rng() % 7), -3);
        const double sg = (rng() & 1) ? 1.0 : -1.0;
        const double Jb[4][4] = {{a, 0.5 * a, sg * b, 0.5 * sg * b}, {a, 0.0, sg * b, 0.0}, {a, sg * b, 0.0, 0.0},
                                 {a, -2.0 * a, sg * b, -2.0 * sg * b}};
        double tb[8][6], lb[8][3];
        std::memcpy(tb, te, sizeof(tb));
        std::memcpy(lb, le, sizeof(lb));
        ref[pos].build(Jb[kind], tb[pos], lb[pos]);
        bool nan = false, infv = false;
        for (double v : tb[pos])
        {
          nan = nan || std::isnan(v);
          infv = infv || std::isinf(v);
        }
        if (!nan && !infv)
          return std::printf("FAIL: the flat cell has a finite element matrix\n"), 1;
        with_nan += nan;
        with_inf += infv;
        const Flags f = run_chains(tb, lb);
        ++nbad;
        missed_pair += !f.pair_any_false;
        missed_cell += !f.cell_any_false;
      }
    // a single +inf that reaches the last pivot only: the diagonal entry of facet E_0 (minus side of cell 0, plus side of
    // cell 7) is the border entry z11 alone - row 0 of the chain is an identity row
    for (int side = 0; side < 2; ++side)
    {
      double tb[8][6], lb[8][3];
      std::memcpy(tb, te, sizeof(tb));
      std::memcpy(lb, le, sizeof(lb));
      if (side == 0)
        tb[0][2] = inf;
      else
        tb[7][5] = inf;
      const Flags f = run_chains(tb, lb);
      ++ninf;
      inf_missed_pair += !f.pair_any_false;
      inf_missed_cell += !f.cell_any_false;
    }
  }
  std::printf("draws %d\n", ndraw);
  std::printf("healthy rings flagged            %d\n", healthy_flagged);
  std::printf("flat cell: rings %d (NaN entries in %d, inf entries in %d)   not flagged: pair %d   cell %d\n", nbad,
              with_nan, with_inf, missed_pair, missed_cell);
  std::printf("+inf on the last pivot: rings %d   not flagged: pair %d   cell %d (a > 0 alone: not asserted)\n", ninf,
              inf_missed_pair, inf_missed_cell);
  const bool pass = healthy_flagged == 0 && missed_pair == 0 && missed_cell == 0 && inf_missed_pair == 0 && with_nan > 0
                    && with_inf > 0;
  std::printf("%s\n", pass ? "PASS" : "FAIL");
  return pass ? 0 : 1;
}
} // namespace

int main(int argc, char** argv)
{
  if (argc > 1 && !std::strcmp(argv[1], "degenerate"))
    return degenerate_rings((argc > 2) ? std::atoi(argv[2]) : 200);
  const int nring = (argc > 1) ? std::atoi(argv[1]) : 2000;
  std::mt19937_64 rng(20240611);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  double err_chain_dense_pair = 0.0, err_chain_dense_cell = 0.0, err_chain_pair_cell = 0.0;
  double err_b_ref_pair = 0.0, err_b_ref_cell = 0.0, err_b_pair_cell = 0.0;
  bool all_ok = true;
  for (int it = 0; it < nring; ++it)
  {
    // ---- reduced system: SPD element matrices M M^T + shift, scaled per cell like cells of different size
    double te[8][6], le[8][3];
    for (int i = 0; i < 8; ++i)
    {
      double M[3][3];
      for (auto& row : M)
        for (double& v : row)
          v = U(rng);
      const double sc = std::exp2(2.0 * U(rng));
      for (int h = 0; h < 3; ++h)
      {
        le[i][h] = sc * U(rng);
        for (int g = 0; g <= h; ++g)
        {
          double s = (h == g) ? 0.05 : 0.0;
          for (int q = 0; q < 3; ++q)
            s += M[h][q] * M[g][q];
          te[i][h * (h + 1) / 2 + g] = sc * s;
        }
      }
    }
    double ref[9];
    dense_solve(te, le, ref);
    double scale = 0.0;
    for (double v : ref)
      scale = std::max(scale, std::fabs(v));
    // lane = cell
    double xc[9];
    {
      C8::T t[6], l[3], d, xm, xp;
      C8::mask ok;
      for (int e = 0; e < 6; ++e)
        t[e] = C8::map([&](int i) { return te[i][e]; });
      for (int h = 0; h < 3; ++h)
        l[h] = C8::map([&](int i) { return le[i][h]; });
      eqlb_pair::cell_chain<C8::T, C8>(t, l, d, xm, xp, ok);
      xc[0] = d.v[0];
      for (int i = 0; i < 8; ++i)
      {
        xc[1 + i] = xm.v[i];
        all_ok = all_ok && ok.v[i] && d.v[i] == d.v[0] && xp.v[i] == xm.v[(i + 1) % 8];
      }
    }
    // two cells per lane
    double xq[9];
    {
      Q4::T t[2][6], l[2][3], d, xe, xo, xn;
      Q4::mask ok;
      for (int c = 0; c < 2; ++c)
      {
        for (int e = 0; e < 6; ++e)
          t[c][e] = Q4::map([&](int i) { return te[2 * i + c][e]; });
        for (int h = 0; h < 3; ++h)
          l[c][h] = Q4::map([&](int i) { return le[2 * i + c][h]; });
      }
      eqlb_pair::pair_chain<Q4::T, Q4>(t, l, d, xe, xo, xn, ok);
      xq[0] = d.v[0];
      for (int i = 0; i < 4; ++i)
      {
        xq[1 + 2 * i] = xe.v[i];
        xq[2 + 2 * i] = xo.v[i];
        all_ok = all_ok && ok.v[i] && d.v[i] == d.v[0] && xn.v[i] == xe.v[(i + 1) % 4];
      }
    }
    for (int j = 0; j < 9; ++j)
    {
      err_chain_dense_pair = std::max(err_chain_dense_pair, std::fabs(xq[j] - ref[j]) / scale);
      err_chain_dense_cell = std::max(err_chain_dense_cell, std::fabs(xc[j] - ref[j]) / scale);
      err_chain_pair_cell = std::max(err_chain_pair_cell, std::fabs(xq[j] - xc[j]) / scale);
    }

    // ---- phase B
    double gm[8][2], gp[8][2], sr0[8];
    bool rm[8], rp[8];
    for (int i = 0; i < 8; ++i)
    {
      for (int j = 0; j < 2; ++j)
      {
        gm[i][j] = U(rng);
        gp[i][j] = U(rng);
      }
      sr0[i] = U(rng);
      rm[i] = (rng() & 1) != 0;
      rp[i] = (rng() & 1) != 0;
    }
    double mm_ref[8][2], mp_ref[8], jv[8][2], tsum[8];
    for (int i = 0; i < 8; ++i)
    {
      double y0, y1;
      rev2_ref(gm[(i + 1) % 8][0], gm[(i + 1) % 8][1], rp[i], y0, y1);
      jv[i][0] = gp[i][0] + y0;
      jv[i][1] = gp[i][1] + y1;
    }
    double bscale = 0.0;
    for (int i = 0; i < 8; ++i)
    {
      tsum[i] = (i ? tsum[i - 1] : 0.0) + sr0[i] + jv[(i + 7) % 8][0];
      mp_ref[i] = tsum[i];
      bscale = std::max(bscale, std::fabs(tsum[i]));
    }
    for (int i = 0; i < 8; ++i)
    {
      const int p = (i + 7) % 8;
      double y0, y1;
      rev2_ref(tsum[p] + jv[p][0], jv[p][1], rm[i], y0, y1);
      mm_ref[i][0] = -y0;
      mm_ref[i][1] = -y1;
      bscale = std::max({bscale, std::fabs(y0), std::fabs(y1)});
    }
    double mm_c[8][2], mp_c[8], mm_q[8][2], mp_q[8];
    {
      C8::T g[2], p[2], mu_m[2], mu_p0;
      for (int j = 0; j < 2; ++j)
      {
        g[j] = C8::map([&](int i) { return gm[i][j]; });
        p[j] = C8::map([&](int i) { return gp[i][j]; });
      }
      eqlb_pair::cell_phase_b<C8::T, C8>(g, p, C8::map([&](int i) { return rm[i] ? 1.0 : 0.0; }),
                                         C8::map([&](int i) { return rp[i] ? 1.0 : 0.0; }),
                                         C8::map([&](int i) { return sr0[i]; }), mu_m, mu_p0);
      for (int i = 0; i < 8; ++i)
      {
        mp_c[i] = mu_p0.v[i];
        mm_c[i][0] = mu_m[0].v[i];
        mm_c[i][1] = mu_m[1].v[i];
      }
    }
    {
      Q4::T g[2][2], p[2][2], r_m[2], r_p[2], s[2], mu_m[2][2], mu_p0[2];
      for (int c = 0; c < 2; ++c)
      {
        for (int j = 0; j < 2; ++j)
        {
          g[c][j] = Q4::map([&](int i) { return gm[2 * i + c][j]; });
          p[c][j] = Q4::map([&](int i) { return gp[2 * i + c][j]; });
        }
        r_m[c] = Q4::map([&](int i) { return rm[2 * i + c] ? 1.0 : 0.0; });
        r_p[c] = Q4::map([&](int i) { return rp[2 * i + c] ? 1.0 : 0.0; });
        s[c] = Q4::map([&](int i) { return sr0[2 * i + c]; });
      }
      eqlb_pair::pair_phase_b<Q4::T, Q4>(g, p, r_m, r_p, s, mu_m, mu_p0);
      for (int i = 0; i < 4; ++i)
        for (int c = 0; c < 2; ++c)
        {
          mp_q[2 * i + c] = mu_p0[c].v[i];
          mm_q[2 * i + c][0] = mu_m[c][0].v[i];
          mm_q[2 * i + c][1] = mu_m[c][1].v[i];
        }
    }
    for (int i = 0; i < 8; ++i)
    {
      const double eq = std::max({std::fabs(mp_q[i] - mp_ref[i]), std::fabs(mm_q[i][0] - mm_ref[i][0]),
                                  std::fabs(mm_q[i][1] - mm_ref[i][1])});
      const double ec = std::max({std::fabs(mp_c[i] - mp_ref[i]), std::fabs(mm_c[i][0] - mm_ref[i][0]),
                                  std::fabs(mm_c[i][1] - mm_ref[i][1])});
      const double eqc = std::max({std::fabs(mp_q[i] - mp_c[i]), std::fabs(mm_q[i][0] - mm_c[i][0]),
                                   std::fabs(mm_q[i][1] - mm_c[i][1])});
      err_b_ref_pair = std::max(err_b_ref_pair, eq / bscale);
      err_b_ref_cell = std::max(err_b_ref_cell, ec / bscale);
      err_b_pair_cell = std::max(err_b_pair_cell, eqc / bscale);
    }
  }
  // bounds: the chain solves are backward stable eliminations of SPD systems whose condition number the generator keeps
  // below about 1e4 (shift 0.05 on entries of order 1, cell scales within 16): 1e4 x 9 unknowns x 2^-53 = 1e-11; phase
  // B is 8 additions: 16 x 2^-53 relative to the largest value
  const double tol_chain = 1e-11, tol_b = 2e-15;
  std::printf("rings %d\n", nring);
  std::printf("chain   pair - dense %.3e   cell - dense %.3e   pair - cell %.3e   (bound %.1e)\n", err_chain_dense_pair,
              err_chain_dense_cell, err_chain_pair_cell, tol_chain);
  std::printf("phase B pair - ring  %.3e   cell - ring  %.3e   pair - cell %.3e   (bound %.1e)\n", err_b_ref_pair,
              err_b_ref_cell, err_b_pair_cell, tol_b);
  const bool pass = all_ok && err_chain_dense_pair <= tol_chain && err_chain_dense_cell <= tol_chain
                    && err_chain_pair_cell <= tol_chain && err_b_ref_pair <= tol_b && err_b_ref_cell <= tol_b
                    && err_b_pair_cell <= tol_b;
  std::printf("%s\n", pass ? "PASS" : "FAIL");
  return pass ? 0 : 1;
}
