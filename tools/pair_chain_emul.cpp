// Host emulation of the lane arithmetic of the RT_2 full-patch body (dolfinx_eqlb_amd/csrc/eqlb_pair_chain.h):
// the pair-lane mapping (4 lanes, two ring cells each) and the lane = cell mapping (8 lanes) run from the same
// templates with the lanes of a patch emulated as array indices, on the same random rings of 8 cells, and are compared
// with each other and with a dense solve / a sequential walk round the ring.
//
//   c++ -O1 -g -std=c++17 [-fsanitize=address,undefined] tools/pair_chain_emul.cpp -o pair_chain_emul && ./pair_chain_emul
//
// exit status 0: every ring within the bounds (printed).  No GPU, no HIP.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
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
  static mask pos(const T& a)
  {
    mask m;
    for (int i = 0; i < N; ++i)
      m.v[i] = a.v[i] > 0.0;
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
using C8 = Lanes<8>;

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
} // namespace

int main(int argc, char** argv)
{
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
