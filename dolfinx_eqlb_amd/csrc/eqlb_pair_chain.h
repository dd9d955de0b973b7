// Lane arithmetic of the RT_2 patch body for a full 8-cell patch, written once for the device and for a host emulation.
//
// The patch is a ring of 8 cells; cell i has the minus facet E_i and the plus facet E_{i+1} (E_8 = E_0).  Two mappings:
//   pair_*  four lanes per patch, lane l holds the ring cells 2 l ("cell 0 of the lane") and 2 l + 1 ("cell 1"): the
//           facet E_{2l+1} is interior to the lane, only E_{2l} and E_{2l+2} are exchanged with the neighbour lanes;
//   cell_*  eight lanes per patch, lane i holds cell i: the arithmetic of se_patch_body (eqlb_se_body.h, K = 2,
//           FULL) restated over the same primitives, as the yardstick of the emulation.
// T is the value type of one register across the lanes (device: double, host: an array indexed by the lane), X the
// lane exchange: X::dn(v) / X::up(v) the value of the previous / next lane of the group (cyclic), X::dn2(v) of the
// lane two places away, X::b0(v) of lane 0, X::qsum(v) the sum over the group in every lane, X::z0(v) / X::z01(v) /
// X::z3(v) the value with an exact zero in lane 0 / lanes 0 and 1 / lane 3, X::one0(v) with 1.0 in lane 0.
// No HIP header is needed: tools/pair_chain_emul.cpp compiles this file with a host compiler.
#pragma once

#ifndef EQLB_PC_FN
#if defined(__HIPCC__)
#define EQLB_PC_FN __device__ __forceinline__
#else
#define EQLB_PC_FN inline
#endif
#endif

namespace eqlb_pair
{

// y = (reversed ? B : I) x for two moments, as reversal_apply<2>: y_0 = x_0, y_1 = x_1 + rho (x_0 - 2 x_1)
template <class T, class X>
EQLB_PC_FN void rev2(const T& x0, const T& x1, const T& rho, T& y0, T& y1)
{
  y0 = x0;
  y1 = X::fma(rho, X::fma(X::cst(-2.0), x1, x0), x1);
}

// ---- phase B: particular solution in own-frame outward moments ------------------------------------------------
// gm / gp [cell][j]: moments of hat G on the minus / plus facet (scaled by pf), rho_m / rho_p [cell]: 1 where the cell
// sees the facet reversed, sr0 [cell]: sgn R_0.  Out: mu_m [cell][j], mu_p0 [cell] (the first moments mu_p[1] are zero)
template <class T, class X>
EQLB_PC_FN void pair_phase_b(const T (&gm)[2][2], const T (&gp)[2][2], const T (&rho_m)[2], const T (&rho_p)[2],
                             const T (&sr0)[2], T (&mu_m)[2][2], T (&mu_p0)[2])
{
  // jump moments on the plus facets: the lane-interior facet from registers, the other from the next lane
  T j0[2], j1[2], t0_, t1_;
  rev2<T, X>(gm[1][0], gm[1][1], rho_p[0], t0_, t1_);
  j0[0] = gp[0][0] + t0_;
  j0[1] = gp[0][1] + t1_;
  const T gn0 = X::up(gm[0][0]), gn1 = X::up(gm[0][1]);
  rev2<T, X>(gn0, gn1, rho_p[1], t0_, t1_);
  j1[0] = gp[1][0] + t0_;
  j1[1] = gp[1][1] + t1_;
  // zero-order chain: inclusive prefix sum of R_0 + J_0(previous facet) round the ring, two cells per step
  const T a0 = sr0[0] + X::dn(j1[0]);
  const T a1 = sr0[1] + j0[0];
  T s = a0 + a1;
  s = s + X::z0(X::dn(s));
  s = s + X::z01(X::dn2(s));
  const T e = X::z0(X::dn(s));
  const T t0 = e + a0, t1 = t0 + a1;
  mu_p0[0] = t0;
  mu_p0[1] = t1;
  // minus facets: the negative of what the previous cell puts on the facet, in the own frame
  T v0, v1;
  rev2<T, X>(X::dn(t1 + j1[0]), X::dn(j1[1]), rho_m[0], v0, v1);
  mu_m[0][0] = -v0;
  mu_m[0][1] = -v1;
  rev2<T, X>(t0 + j0[0], j0[1], rho_m[1], v0, v1);
  mu_m[1][0] = -v0;
  mu_m[1][1] = -v1;
}

// the same with one cell per lane (8 lanes; X::dn / X::up cyclic over the 8 lanes, X::pre(v, S) the value of lane
// i - S or an exact zero for i < S)
template <class T, class X>
EQLB_PC_FN void cell_phase_b(const T (&gm)[2], const T (&gp)[2], const T& rho_m, const T& rho_p, const T& sr0,
                             T (&mu_m)[2], T& mu_p0)
{
  T jv[2], t0_, t1_;
  rev2<T, X>(X::up(gm[0]), X::up(gm[1]), rho_p, t0_, t1_);
  jv[0] = gp[0] + t0_;
  jv[1] = gp[1] + t1_;
  T t = sr0 + X::dn(jv[0]);
  t = t + X::pre(t, 1);
  t = t + X::pre(t, 2);
  t = t + X::pre(t, 4);
  mu_p0 = t;
  T v0, v1;
  rev2<T, X>(X::dn(t + jv[0]), X::dn(jv[1]), rho_m, v0, v1);
  mu_m[0] = -v0;
  mu_m[1] = -v1;
}

// ---- reduced system: border [d ; x_0] + scalar tridiagonal chain x_1 .. x_7 -----------------------------------
// te [cell][6]: lower triangle of the element matrix in the local unknowns [d | um | up] (entry h (h + 1) / 2 + g),
// le [cell][3]: its load.  Out: d, xe = x_{2l}, xo = x_{2l+1}, xn = x_{2l+2}; ok: every pivot positive.
// The even rows (facets E_{2l}) are eliminated first - their coupling to the odd row of the lane is register
// arithmetic, the one to the odd row of the previous lane one exchange - which leaves one row per lane: two levels of
// parallel cyclic reduction over the 4 lanes (in the second the rows l - 2 and l + 2 are the same lane).  Row 0 is the
// border row and an identity row of the chain; couplings across the ends are exact zeros, so what the cyclic
// exchanges drag round the ring is multiplied by zero (as in se_patch_body).
template <class T, class X>
EQLB_PC_FN void pair_chain(const T (&te)[2][6], const T (&le)[2][3], T& d, T& xe, T& xo, T& xn, typename X::mask& ok)
{
  const T alpha = X::qsum(te[0][0] + te[1][0]), rd = X::qsum(le[0][0] + le[1][0]);
  // block rows of the facets: own minus-side entries + plus-side entries of the previous cell
  const T bt_e = te[0][1] + X::dn(te[1][3]), rr_e = le[0][1] + X::dn(le[1][2]), dg_e = te[0][2] + X::dn(te[1][5]);
  const T bt_o = te[1][1] + te[0][3], rr_o = le[1][1] + le[0][2], dg_o = te[1][2] + te[0][5];
  const T off_e = te[0][4], off_o = te[1][4];
  // border data (row of E_0: the even row of lane 0)
  const T z10 = X::b0(bt_e), z11 = X::b0(dg_e), rz1 = X::b0(rr_e);
  // chain rows: right-hand sides [rr | column of d | column of x_0]
  const T be = X::one0(dg_e), re0 = X::z0(rr_e), re1 = X::z0(bt_e); // (third column of an even row: zero)
  const T ce = X::z0(off_e);                                         // coupling E_{2l} - E_{2l+1}
  const T co = X::z3(off_o);                                         // coupling E_{2l+1} - E_{2l+2}
  const T c0 = X::only0(off_e) + X::only3(off_o);                    // coupling of x_1 and of x_7 (wrapping) to x_0
  // elimination of the even rows
  ok = X::pos(be);
  const T ibe = X::rcp(be);
  const T ibe_up = X::up(ibe), re0_up = X::up(re0), re1_up = X::up(re1), co_dn = X::dn(co);
  const T fe = ce * ibe, fh = co * ibe_up;
  T b = X::fma(-fh, co, X::fma(-fe, ce, dg_o));
  T r0 = X::fma(-fh, re0_up, X::fma(-fe, re0, rr_o));
  T r1 = X::fma(-fh, re1_up, X::fma(-fe, re1, bt_o));
  T r2 = c0;
  T am = -fe * co_dn; // coupling of the odd row to the odd row of the previous lane
  // level 1
  {
    ok = X::both(ok, X::pos(b));
    const T ib = X::rcp(b);
    const T ib_lo = X::dn(ib), a_lo = X::dn(am), r0_lo = X::dn(r0), r1_lo = X::dn(r1), r2_lo = X::dn(r2);
    const T ib_hi = X::up(ib), cp = X::up(am), r0_hi = X::up(r0), r1_hi = X::up(r1), r2_hi = X::up(r2);
    const T al = am * ib_lo, ga = cp * ib_hi;
    b = X::fma(-ga, cp, X::fma(-al, am, b));
    r0 = X::fma(-ga, r0_hi, X::fma(-al, r0_lo, r0));
    r1 = X::fma(-ga, r1_hi, X::fma(-al, r1_lo, r1));
    r2 = X::fma(-ga, r2_hi, X::fma(-al, r2_lo, r2));
    am = -al * a_lo;
  }
  // level 2: am is the coupling to row l - 2 (lanes 2, 3), the coupling to row l + 2 is am of that lane (lanes 0, 1)
  {
    ok = X::both(ok, X::pos(b));
    const T ib = X::rcp(b);
    const T ib2 = X::dn2(ib), cp = X::dn2(am), r0_2 = X::dn2(r0), r1_2 = X::dn2(r1), r2_2 = X::dn2(r2);
    const T al = am * ib2, ga = cp * ib2;
    b = X::fma(-ga, cp, X::fma(-al, am, b));
    const T w = al + ga;
    r0 = X::fma(-w, r0_2, r0);
    r1 = X::fma(-w, r1_2, r1);
    r2 = X::fma(-w, r2_2, r2);
  }
  ok = X::both(ok, X::pos(b));
  const T ibf = X::rcp(b);
  const T so0 = r0 * ibf, so1 = r1 * ibf, so2 = r2 * ibf; // A^-1 [rr | bt | c0], odd rows
  // even rows by back substitution
  const T se0 = ibe * X::fma(-ce, so0, X::fma(-co_dn, X::dn(so0), re0));
  const T se1 = ibe * X::fma(-ce, so1, X::fma(-co_dn, X::dn(so1), re1));
  const T se2 = -ibe * X::fma(ce, so2, co_dn * X::dn(so2));
  // Schur complement of the chain on the border
  const T tred0 = X::qsum(X::fma(re1, se0, bt_o * so0)), tred1 = X::qsum(c0 * so0);
  const T s00 = X::qsum(X::fma(re1, se1, bt_o * so1)), s10 = X::qsum(c0 * so1), s11 = X::qsum(c0 * so2);
  const T l00 = alpha - s00, l10 = z10 - s10;
  const T i0 = X::rcp(l00);
  const T m = l10 * i0;
  const T d1 = X::fma(-m, l10, z11 - s11);
  ok = X::both(ok, X::both(X::pos(l00), X::pos(d1)));
  const T q0 = rd - tred0;
  const T q1 = X::fma(-m, q0, rz1 - tred1);
  const T zz1 = q1 * X::rcp(d1);
  const T zz0 = X::fma(-l10, zz1, q0) * i0;
  d = zz0;
  xo = X::fma(-so2, zz1, X::fma(-so1, zz0, so0));
  xe = X::sel0(zz1, X::fma(-se2, zz1, X::fma(-se1, zz0, se0)));
  xn = X::up(xe);
}

// the same with one cell per lane: se_patch_body, SOLVER 1, K = 2, P = 8, FULL (three levels over 8 lanes; X::shr(v, S)
// / X::shl(v, S): the value of lane i - S / i + S, an exact zero outside the group; X::gsum the sum over the 8 lanes).
// Out: d, xm = x_i, xp = x_{i+1}
template <class T, class X>
EQLB_PC_FN void cell_chain(const T (&te)[6], const T (&le)[3], T& d, T& xm, T& xp, typename X::mask& ok)
{
  const T alpha = X::gsum(te[0]), rd = X::gsum(le[0]);
  const T bt = te[1] + X::dn(te[3]), rr = le[1] + X::dn(le[2]), dg = te[2] + X::dn(te[5]), off = te[4];
  const T z10 = X::b0(bt), z11 = X::b0(dg), rz1 = X::b0(rr), off0 = X::b0(off);
  // chain rows 1 .. 7 (row 0: identity), OffC zero in the wrapping row 7
  T b = X::one0(dg), r0 = X::z0(rr), r1 = X::z0(bt);
  const T offc = X::z0(X::zlast(off));
  T r2 = X::only1(off0) + X::onlylast(off);
  const T B1 = r1, B2 = r2;
  T am = X::shr(offc, 1);
  ok = X::pos(b);
  for (int S = 1; S < 8; S *= 2)
  {
    ok = X::both(ok, X::pos(b));
    const T ib = X::rcp(b);
    const T ib_lo = X::shr(ib, S), a_lo = X::shr(am, S), r0_lo = X::shr(r0, S), r1_lo = X::shr(r1, S),
            r2_lo = X::shr(r2, S);
    const T ib_hi = X::shl(ib, S), cp = X::shl(am, S), r0_hi = X::shl(r0, S), r1_hi = X::shl(r1, S),
            r2_hi = X::shl(r2, S);
    const T al = am * ib_lo, ga = cp * ib_hi;
    b = X::fma(-ga, cp, X::fma(-al, am, b));
    r0 = X::fma(-ga, r0_hi, X::fma(-al, r0_lo, r0));
    r1 = X::fma(-ga, r1_hi, X::fma(-al, r1_lo, r1));
    r2 = X::fma(-ga, r2_hi, X::fma(-al, r2_lo, r2));
    am = -al * a_lo;
  }
  ok = X::both(ok, X::pos(b));
  const T ibf = X::rcp(b);
  const T s0 = r0 * ibf, s1 = r1 * ibf, s2 = r2 * ibf;
  const T tred0 = X::gsum(B1 * s0), tred1 = X::gsum(B2 * s0);
  const T s00 = X::gsum(B1 * s1), s10 = X::gsum(B2 * s1), s11 = X::gsum(B2 * s2);
  const T l00 = alpha - s00, l10 = z10 - s10;
  const T i0 = X::rcp(l00);
  const T m = l10 * i0;
  const T d1 = X::fma(-m, l10, z11 - s11);
  ok = X::both(ok, X::both(X::pos(l00), X::pos(d1)));
  const T q0 = rd - tred0;
  const T q1 = X::fma(-m, q0, rz1 - tred1);
  const T zz1 = q1 * X::rcp(d1);
  const T zz0 = X::fma(-l10, zz1, q0) * i0;
  d = zz0;
  xm = X::sel0(zz1, X::fma(-s2, zz1, X::fma(-s1, zz0, s0)));
  xp = X::up(xm);
}

} // namespace eqlb_pair
