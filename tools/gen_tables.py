#!/usr/bin/env python3
"""Generate the constant reference-cell tensors of the HIP equilibration kernels.

The reference evaluates every patch integral by runtime quadrature over Basix tabulations
(cpp/dolfinx_eqlb/se/KernelData.cpp, se/fluxmin_kernel.hpp:94-174,
se/solve_patch_semiexplt.hpp:645-934).  On affine cells all of these integrals are linear
combinations of a few constant tensors on the reference triangle; they are computed here in
exact rational arithmetic and emitted as `double` literals, so the device code needs neither
Basix nor quadrature loops:

  S[3][nd_rt][nd_rt]   S0 = int phi_i^x phi_j^x, S1 = int phi_i^x phi_j^y + phi_i^y phi_j^x,
                       S2 = int phi_i^y phi_j^y   (hierarchic RT_k basis, e_raviart_thomas.py)
                       physical mass matrix = (g00 S0 + g01 S1 + g11 S2)/|detJ|,  g = J^T J
  F[3][3][nd][k]       int_0^1 psi_i(x_f(s)) hat_n(x_f(s)) s^j ds   (facet moments of hat*G)
  H[3][nd][nq]         int_T psi_i hat_n mono_q          (mono_0 = 1, then the div-moment x^l y^m)
  D[3][nd][2][nq]      int_T d_X psi_i hat_n mono_q
  B[k][k]              B_ji = C(j,i)(-1)^i : moments w.r.t. s of a trace given by its moments
                       w.r.t. 1-s (reversed facet), cf. se/KernelData.cpp:49-64
  NREF[3][2], NOUT[3]  reference facet normals of the RT functionals and their outwardness
  PG[2][nd_d][nd_p]    projected reference gradient of a P_p function in DG_d (eqlb_primal_flux.hip): the DG_d nodal
                       values of d/dX phi_i for d >= p-1 (exact), Minv_d int psi_n d/dX phi_i (L2 projection) below
  PT[(2q+1)(q+1)][nd_q] values of the P_q basis functions at the half-spacing lattice of the reference triangle, the
                       prolongation across one bisection level (eqlb_transfer.hip; the lattice and its row order:
                       dolfinx_eqlb_amd/mesh/transfer.py)
  FB[6][k][k]          facet DOFs of a flux boundary condition on a child facet from those of its parent, one matrix
                       per map of the facet parameter (eqlb_bc_carry.hip; mesh/transfer.py: flux_bc_table_exact)
  ST[3][nd_p][nd_p]    reference stiffness of P_p: int dX phi_i dX phi_j, int (dX phi_i dY phi_j + dY phi_i dX phi_j),
                       int dY phi_i dY phi_j (eqlb_primal_solve.hip; lsolver/primal.py: stiffness_table_exact)
  LD[nd_p][nd_d]       int phi_i chi_n, chi_n the DG_d nodal basis: the load of P_p against DG_d data (load_table_exact)
  CR[nd_p][nd_p]       int dX phi_i dY phi_j: with ST the four reference blocks of the elasticity operator
                       (eqlb_primal_elasticity.hip; lsolver/primal.py: cross_table_exact)
  MS[nd_p][nd_p]       int phi_i phi_j: the reaction term of both operators (lsolver/primal.py: mass_table_exact)
  PV[nd_d][nd_p]       DG_d nodal values of the L2 projection of phi_i onto P_d: interpolation for d >= p,
                       MS<d>^-1 LD<p,d>^T below (eqlb_primal_flux.hip: eqlb_primal_value_dg; value_table_exact)

Run:  python tools/gen_tables.py   (rewrites dolfinx_eqlb_amd/csrc/eqlb_tables_gen.h; the pairs of PAIRS_BUILD
      go to the header `python tools/gen_tables.py --build PATH` writes, which the build runs)
"""

import os
import sys
from fractions import Fraction
from math import comb

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from dolfinx_eqlb_amd.elmtlib import polynomials as P  # noqa: E402
from dolfinx_eqlb_amd.elmtlib import e_raviart_thomas as ert  # noqa: E402
from dolfinx_eqlb_amd.elmtlib.lagrange import Lagrange  # noqa: E402

PAIRS = [(1, 0), (2, 1), (3, 2), (4, 3), (2, 0), (3, 1), (3, 0)]  # (k, degree of DG data)
# RT_4 with data of degree < 3: 0.4 MB of literals, generated at build time (csrc/Makefile, `--build`) into
# eqlb_tables_build_gen.h, which git ignores
PAIRS_BUILD = [(4, 2), (4, 1), (4, 0)]
NCOMBO = 12  # (fm, fp, rev) combinations with fm != fp
# (degree p of the primal P_p solution, degree d of the projected flux) of the PG tables
PAIRS_PRIMAL = [(p, d) for p in range(1, 5) for d in range(4)]


def combo(fm, fp, rev):
    """Row of the reduced tensors: the six ordered pairs of distinct local facet ids x reversal."""
    return (fm * 2 + (fp if fp < fm else fp - 1)) * 2 + rev


def tables_exact(k, deg):
    rt = ert.HierarchicRT(k)
    dg = Lagrange(deg)
    hat = Lagrange(1)
    nrt, nd = rt.ndofs, dg.ndofs
    monos = [(0, 0)] + rt.div_exponents
    S = [[[Fraction(0)] * nrt for _ in range(nrt)] for _ in range(3)]
    for i in range(nrt):
        for j in range(nrt):
            xi, yi = rt.basis[i]
            xj, yj = rt.basis[j]
            S[0][i][j] = P.integrate_triangle(P.mul(xi, xj))
            S[1][i][j] = P.integrate_triangle(P.mul(xi, yj)) + P.integrate_triangle(P.mul(yi, xj))
            S[2][i][j] = P.integrate_triangle(P.mul(yi, yj))
    # component-wise products for the stress estimator (tr^2, asymmetry): SU0 = int phi_i^x phi_j^x,
    # SU1 = int phi_i^x phi_j^y (not symmetrised), SU2 = int phi_i^y phi_j^y
    SU = [[[P.integrate_triangle(P.mul(rt.basis[i][a], rt.basis[j][b])) for j in range(nrt)] for i in range(nrt)]
          for (a, b) in ((0, 0), (0, 1), (1, 1))]
    F = [[[[Fraction(0)] * k for _ in range(nd)] for _ in range(3)] for _ in range(3)]
    for f in range(3):
        xs, ys = ert.FACET_PARAM[f]
        for n in range(3):
            for i in range(nd):
                tr = P.restrict_to_line(P.mul(dg.basis[i], hat.basis[n]), xs, ys)
                for j in range(k):
                    F[f][n][i][j] = P.integrate_unit_interval(tr, j)
    H = [[[Fraction(0)] * len(monos) for _ in range(nd)] for _ in range(3)]
    D = [[[[Fraction(0)] * len(monos) for _ in range(2)] for _ in range(nd)] for _ in range(3)]
    for n in range(3):
        for i in range(nd):
            for q, (l, m) in enumerate(monos):
                w = P.mul(hat.basis[n], P.monomial(l, m))
                H[n][i][q] = P.integrate_triangle(P.mul(dg.basis[i], w))
                D[n][i][0][q] = P.integrate_triangle(P.mul(P.ddx(dg.basis[i]), w))
                D[n][i][1][q] = P.integrate_triangle(P.mul(P.ddy(dg.basis[i]), w))
    B = [[Fraction(comb(j, i) * (-1) ** i) for i in range(k)] for j in range(k)]
    TE, WQ = reduced_tensors(k, S, B)
    # weak symmetry: V[j][i][X] = int hat_j phi_i^X, and its reduction to the local H(div=0)
    # functions per combination: VQ[ci][X][h][j] = sum_r Q[r][h] D0_r V[j][idx_r][X]
    V = [[[P.integrate_triangle(P.mul(hat.basis[j], rt.basis[i][X])) for X in range(2)]
          for i in range(nrt)] for j in range(3)]
    VQ = reduced_symmetry_tensor(k, V, B)
    # per-patch flux-BC DOFs (BoundaryData::calculate_patch_bc): moments of hat_n * g on facet f from
    # the moments b_j of g: HB[f][n][i][j] = int_0^1 p_j(s) hat_n(x_f(s)) s^i ds, int p_j s^i = delta_ij
    hil = [[Fraction(1, i + m + 1) for m in range(k)] for i in range(k)]
    hinv = P.solve_exact(hil, [[Fraction(int(i == j)) for j in range(k)] for i in range(k)])
    HB = [[[[Fraction(0)] * k for _ in range(k)] for _ in range(3)] for _ in range(3)]
    for f in range(3):
        xs, ys = ert.FACET_PARAM[f]
        for n in range(3):
            hl = P.restrict_to_line(hat.basis[n], xs, ys)
            for j in range(k):
                pj = [hinv[j][m] for m in range(k)]  # coefficients of p_j (H symmetric)
                prod = P._poly1d_mul(pj, hl)
                for i in range(k):
                    HB[f][n][i][j] = P.integrate_unit_interval(prod, i)
    # constrained-minimisation (EV) equilibrator: HG[i][q] = int psi_i mono_q (moments of
    # grad hat . G), WGF[n][i][d][c] = int hat_n psi_d phi_i^c (linear term (phi_i, hat_n G)) and its
    # reduction WG[ci][h][d][c] = sum_r Q[r][h] D0_r WGF[ln][idx_r][d][c], ln = 3 - fm - fp
    HG = [[P.integrate_triangle(P.mul(dg.basis[i], P.monomial(l, m))) for (l, m) in monos]
          for i in range(nd)]
    WGF = [[[[P.integrate_triangle(P.mul(P.mul(hat.basis[n], dg.basis[d]), rt.basis[i][c]))
              for c in range(2)] for d in range(nd)] for i in range(nrt)] for n in range(3)]
    nh = 1 + 2 * (k - 1) + (k - 1) * (k - 2) // 2
    WG = [[[[Fraction(0)] * 2 for _ in range(nd)] for _ in range(nh)] for _ in range(NCOMBO)]
    for fm in range(3):
        for fp in range(3):
            if fm == fp:
                continue
            ln = 3 - fm - fp
            for rev in range(2):
                ci = combo(fm, fp, rev)
                idx, d0, Q, ny, nh_ = _local_maps(k, B, fm, fp, rev)
                for h in range(nh):
                    for d in range(nd):
                        for c in range(2):
                            WG[ci][h][d][c] = sum(Q[r][h] * d0[r] * WGF[ln][idx[r]][d][c]
                                                  for r in range(ny))
    # acceptance / estimator step on the device (eqlb_estimate.hip): moments of grad psi_i against
    # the monomials, inverse Gram matrix of the monomials, facet moments of psi_i (no hat)
    nq_ = len(monos)
    DM = [[[P.integrate_triangle(P.mul(d(dg.basis[i]), P.monomial(l, m))) for (l, m) in monos]
           for d in (P.ddx, P.ddy)] for i in range(nd)]
    gram = [[P.integrate_triangle(P.mul(P.monomial(*monos[a]), P.monomial(*monos[b])))
             for b in range(nq_)] for a in range(nq_)]
    GMI = P.solve_exact(gram, [[Fraction(int(a == b)) for b in range(nq_)] for a in range(nq_)])
    F0 = [[[sum(F[f][n][i][j] for n in range(3)) for j in range(k)] for i in range(nd)]
          for f in range(3)]
    # flux part of the estimator for a flux sigma given next to the discrete flux G (EV):
    # MRD[i][d][c] = int phi_i^c psi_d, MPS[d][e] = int psi_d psi_e
    MRD = [[[P.integrate_triangle(P.mul(rt.basis[i][c], dg.basis[d])) for c in range(2)]
            for d in range(nd)] for i in range(nrt)]
    MPS = [[P.integrate_triangle(P.mul(dg.basis[d], dg.basis[e])) for e in range(nd)] for d in range(nd)]
    return dict(k=k, deg=deg, nrt=nrt, nd=nd, nq=len(monos), S=S, F=F, H=H, D=D, B=B, TE=TE, WQ=WQ,
                V=V, VQ=VQ, HB=HB, HG=HG, WGF=WGF, WG=WG, DM=DM, GMI=GMI, F0=F0, MRD=MRD, MPS=MPS, SU=SU,
                monos=monos)


def _local_maps(k, B, fm, fp, rev):
    """(idx_y, d0, Q) of a facet-pair combination: own-frame unknowns y = [mu_m | mu_p | add],
    c = sgn * D0 y, y = ytil + Q [d | um | up | ua] (see reduced_tensors)."""
    kb = k - 1
    nadd = (k - 1) * (k - 2) // 2
    ndiv = k * (k + 1) // 2 - 1
    ny, nh = 2 * k + nadd, 1 + 2 * kb + nadd
    zero = Fraction(0)
    idx = [fm * k + j for j in range(k)] + [fp * k + j for j in range(k)] \
        + [3 * k + ndiv + q for q in range(nadd)]
    sm = 1 if ert.FACET_NORMAL_IS_OUTWARD[fm] else -1
    sp = 1 if ert.FACET_NORMAL_IS_OUTWARD[fp] else -1
    d0 = [sm] * k + [sp] * k + [1] * nadd
    Q = [[zero] * nh for _ in range(ny)]
    for j in range(k):
        for c in range(k):
            Q[j][c] = -(B[j][c] if rev else Fraction(int(j == c)))
    Q[k][0] = Fraction(1)
    for j in range(1, k):
        Q[k + j][kb + j] = Fraction(1)
    for q in range(nadd):
        Q[2 * k + q][1 + 2 * kb + q] = Fraction(1)
    return idx, d0, Q, ny, nh


def reduced_symmetry_tensor(k, V, B):
    zero = Fraction(0)
    nh = 1 + 2 * (k - 1) + (k - 1) * (k - 2) // 2
    VQ = [[[[zero] * 3 for _ in range(nh)] for _ in range(2)] for _ in range(NCOMBO)]
    for fm in range(3):
        for fp in range(3):
            if fm == fp:
                continue
            for rev in range(2):
                ci = combo(fm, fp, rev)
                idx, d0, Q, ny, nh_ = _local_maps(k, B, fm, fp, rev)
                for X in range(2):
                    for h in range(nh):
                        for j in range(3):
                            VQ[ci][X][h][j] = sum(Q[r][h] * d0[r] * V[j][idx[r]][X] for r in range(ny))
    return VQ


def reduced_tensors(k, S, B):
    """Element matrices of the patch-wise H(div=0) functions, per combination
    ci = (fm*3 + fp)*2 + rev of the local ids of the two patch facets of a cell and the
    reversal flag of the minus facet, for the three metric components x:

      TE[ci][x][h(h+1)/2+g] = (Q^T D0 S_x D0 Q)_{hg}          local unknowns [d | um | up | ua]
      WQ[ci][x][h][c]       = (Q^T D0 S_x [D0 | I])_{hc}      columns [mu_m | mu_p | div DOFs]

    with S_x restricted to the DOFs [minus facet | plus facet | interior | div], D0 the signs
    turning outward flux moments into RT coefficients (up to sign(detJ), which cancels), and Q
    the map of se/fluxmin_kernel.hpp:107-138 (d0 function, reversed-facet transformation) in the
    own-frame formulation: mu_m += -Bm [d; um], mu_p += [d; up].
    element matrix = sum_x g_x TE_x, g = J^T J / |detJ|;  load = -sum_x g_x WQ_x [mu_m; mu_p; s c_div].
    """
    kb = k - 1
    nadd = (k - 1) * (k - 2) // 2
    ndiv = k * (k + 1) // 2 - 1
    ny, nh = 2 * k + nadd, 1 + 2 * kb + nadd
    ncol = 2 * k + ndiv
    nte = nh * (nh + 1) // 2
    zero = Fraction(0)
    TE = [[[zero] * nte for _ in range(3)] for _ in range(NCOMBO)]
    WQ = [[[[zero] * ncol for _ in range(nh)] for _ in range(3)] for _ in range(NCOMBO)]
    for fm in range(3):
        for fp in range(3):
            if fm == fp:
                continue
            idx = [fm * k + j for j in range(k)] + [fp * k + j for j in range(k)] \
                + [3 * k + ndiv + q for q in range(nadd)] + [3 * k + q for q in range(ndiv)]
            sm = 1 if ert.FACET_NORMAL_IS_OUTWARD[fm] else -1
            sp = 1 if ert.FACET_NORMAL_IS_OUTWARD[fp] else -1
            d0 = [sm] * k + [sp] * k + [1] * nadd
            for rev in range(2):
                ci = combo(fm, fp, rev)
                Q = [[zero] * nh for _ in range(ny)]
                for j in range(k):
                    for c in range(k):
                        bm = B[j][c] if rev else Fraction(int(j == c))
                        Q[j][c] = -bm  # local unknown c: 0 = d, 1..kb = um
                Q[k][0] = Fraction(1)
                for j in range(1, k):
                    Q[k + j][kb + j] = Fraction(1)
                for q in range(nadd):
                    Q[2 * k + q][1 + 2 * kb + q] = Fraction(1)
                for x in range(3):
                    M = [[S[x][idx[r]][idx[c]] for c in range(len(idx))] for r in range(ny)]
                    # A = D0 M_yy D0 ; columns of the load: [mu_m | mu_p | div]
                    cols = list(range(2 * k)) + list(range(ny, ny + ndiv))
                    dcol = d0[:2 * k] + [1] * ndiv
                    DM = [[d0[r] * M[r][c] for c in range(len(idx))] for r in range(ny)]
                    for h in range(nh):
                        for cc, c in enumerate(cols):
                            WQ[ci][x][h][cc] = sum(Q[r][h] * DM[r][c] * dcol[cc] for r in range(ny))
                        for g in range(h + 1):
                            TE[ci][x][h * (h + 1) // 2 + g] = sum(
                                Q[r][h] * DM[r][c] * d0[c] * Q[c][g] for r in range(ny) for c in range(ny))
    return TE, WQ


def _evaluate_exact(p, x, y):
    return sum((c * x ** a * y ** b for (a, b), c in p.items()), Fraction(0))


def primal_table_exact(p, d):
    """PG[X][n][i]: DG_d DOF n of the projection of d/dX phi_i, phi_i the basis of P_p (Basix numbering of
    elmtlib/lagrange.py for both).  grad_X P_p lies in P_{p-1}^2: for d >= p-1 the projection is the nodal
    interpolation (what embed_dg produces from the DG_{p-1} values), below it is the L2 projection, whose
    |detJ| cancels on an affine cell."""
    el, dg = Lagrange(p), Lagrange(d)
    npp, nd = el.ndofs, dg.ndofs
    grads = [[der(el.basis[i]) for i in range(npp)] for der in (P.ddx, P.ddy)]
    if d >= p - 1:
        return [[[_evaluate_exact(grads[X][i], *dg.nodes[n]) for i in range(npp)] for n in range(nd)]
                for X in range(2)]
    mass = [[P.integrate_triangle(P.mul(dg.basis[i], dg.basis[j])) for j in range(nd)] for i in range(nd)]
    out = []
    for X in range(2):
        load = [[P.integrate_triangle(P.mul(dg.basis[n], grads[X][i])) for i in range(npp)] for n in range(nd)]
        out.append(P.solve_exact(mass, load))
    return out


def primal_table_float(p, d):
    import numpy as np
    nd, npp = (d + 1) * (d + 2) // 2, (p + 1) * (p + 2) // 2
    return np.array([float(v) for v in _flat(primal_table_exact(p, d))]).reshape(2, nd, npp)


def _flat(x):
    if isinstance(x, list):
        for y in x:
            yield from _flat(y)
    else:
        yield x


def tables_float(k, deg):
    """Same tensors as numpy arrays (used by the numpy prototype in tests/)."""
    import numpy as np
    t = tables_exact(k, deg)
    out = dict(k=k, deg=deg, nrt=t["nrt"], nd=t["nd"], nq=t["nq"])
    for name in ("S", "F", "H", "D", "B", "TE", "WQ", "V", "VQ", "HB", "HG", "WGF", "WG", "DM", "GMI",
                 "F0", "MRD", "MPS"):
        def shape(x):
            return (len(x),) + shape(x[0]) if isinstance(x, list) else ()
        out[name] = np.array([float(v) for v in _flat(t[name])]).reshape(shape(t[name]))
    out["NREF"] = np.array(ert.FACET_NORMALS, dtype=float)
    out["NOUT"] = np.array(ert.FACET_NORMAL_IS_OUTWARD, dtype=bool)
    return out


def _emit_refs(lines, pairs):
    for (k, deg) in pairs:
        t = tables_exact(k, deg)
        nrt, nd, nq = t["nrt"], t["nd"], t["nq"]
        lines.append(f"template <> struct Ref<{k}, {deg}> {{")
        lines.append(f"  static constexpr int NRT = {nrt}, ND = {nd}, NQ = {nq};")

        def arr(name, dims, data):
            vals = ", ".join(repr(float(v)) for v in _flat(data))
            d = "".join(f"[{x}]" for x in dims)
            n = 1
            for x in dims:
                n *= x
            lines.append(f"  static constexpr int {name}_SIZE = {n};")
            lines.append(f"  // {name}{d}")
            lines.append(f"  static constexpr double {name}[{n}] = {{{vals}}};")
        arr("S", (3, nrt, nrt), t["S"])
        arr("F", (3, 3, nd, k), t["F"])
        arr("H", (3, nd, nq), t["H"])
        arr("D", (3, nd, 2, nq), t["D"])
        arr("B", (k, k), t["B"])
        kb_, nadd_, ndiv_ = k - 1, (k - 1) * (k - 2) // 2, k * (k + 1) // 2 - 1
        nh_ = 1 + 2 * kb_ + nadd_
        arr("TE", (NCOMBO, 3, nh_ * (nh_ + 1) // 2), t["TE"])
        arr("WQ", (NCOMBO, 3, nh_, 2 * k + ndiv_), t["WQ"])
        arr("V", (3, nrt, 2), t["V"])
        arr("VQ", (NCOMBO, 2, nh_, 3), t["VQ"])
        arr("HB", (3, 3, k, k), t["HB"])
        arr("HG", (nd, nq), t["HG"])
        arr("WG", (NCOMBO, nh_, nd, 2), t["WG"])
        arr("DM", (nd, 2, nq), t["DM"])
        arr("GMI", (nq, nq), t["GMI"])
        arr("F0", (3, nd, k), t["F0"])
        arr("MRD", (nrt, nd, 2), t["MRD"])
        arr("MPS", (nd, nd), t["MPS"])
        arr("SU", (3, nrt, nrt), t["SU"])
        lines.append("  // exponents (l, m) of the monomials x^l y^m the NQ divergence moments are taken with")
        lines.append(f"  static constexpr int MONO_X[{nq}] = {{{', '.join(str(l) for l, _ in t['monos'])}}};")
        lines.append(f"  static constexpr int MONO_Y[{nq}] = {{{', '.join(str(m) for _, m in t['monos'])}}};")
        lines.append("};")
        lines.append("")


def emit(path):
    lines = ["// GENERATED by tools/gen_tables.py - do not edit.",
             "// Exact reference-cell tensors of the hierarchic RT_k / DG_deg pair (see the generator).",
             "#pragma once", "", "namespace eqlb_tables {", "",
             "template <int K, int DEG> struct Ref;", ""]
    _emit_refs(lines, PAIRS)
    # Lagrange P_d (Basix numbering, equispaced): monomial coefficients and inverse mass matrix
    lines.append("// Lagrange P_d on the reference triangle: LAG_COEF[i][m] = coefficient of monomial m")
    lines.append("// (order: deg 0; x, y; x^2, xy, y^2; ...) of basis function i; LAG_MINV = inverse of int psi_i psi_j")
    lines.append("template <int DEG> struct Lag;")
    for deg in range(4):
        dg = Lagrange(deg)
        nd = dg.ndofs
        monos = [(a, d - a) for d in range(deg + 1) for a in range(d, -1, -1)]
        coef = [[dg.basis[i].get(m, Fraction(0)) for m in monos] for i in range(nd)]
        mass = [[P.integrate_triangle(P.mul(dg.basis[i], dg.basis[j])) for j in range(nd)] for i in range(nd)]
        minv = P.solve_exact(mass, [[Fraction(int(i == j)) for j in range(nd)] for i in range(nd)])
        lines.append(f"template <> struct Lag<{deg}> {{")
        lines.append(f"  static constexpr int ND = {nd};")
        lines.append(f"  static constexpr double COEF[{nd * nd}] = {{" + ", ".join(repr(float(v)) for v in _flat(coef)) + "};")
        lines.append(f"  static constexpr double MINV[{nd * nd}] = {{" + ", ".join(repr(float(v)) for v in _flat(minv)) + "};")
        lines.append("};")
    lines.append("")
    lines.append("// projected reference gradient of P_p in DG_d: PG[X][n][i] = DG_d DOF n of d/dX phi_i (nodal values for")
    lines.append("// d >= p-1, L2 projection below); flux_dg = -kappa K^T PG u_cell (eqlb_primal_flux.hip)")
    lines.append("template <int P, int D> struct Primal;")
    for (p, d) in PAIRS_PRIMAL:
        npp, nd = (p + 1) * (p + 2) // 2, (d + 1) * (d + 2) // 2
        lines.append(f"template <> struct Primal<{p}, {d}> {{")
        lines.append(f"  static constexpr int NP = {npp}, ND = {nd};")
        lines.append(f"  static constexpr double PG[{2 * nd * npp}] = {{"
                     + ", ".join(repr(float(v)) for v in _flat(primal_table_exact(p, d))) + "};")
        lines.append("};")
    lines.append("")
    from dolfinx_eqlb_amd.mesh.transfer import prolong_table_exact
    lines.append("// prolongation of P_q across one bisection level: PT[row][k] = basis function k of the equispaced P_q at the")
    lines.append("// lattice point (i, j) / (2q), row = j (2q+1) - j (j-1) / 2 + i (mesh/transfer.py, eqlb_transfer.hip)")
    lines.append("template <int Q> struct Prolong;")
    for q in range(1, 5):
        t = prolong_table_exact(q)
        lines.append(f"template <> struct Prolong<{q}> {{")
        lines.append(f"  static constexpr int NROW = {len(t)}, ND = {len(t[0])};")
        lines.append(f"  static constexpr double PT[{len(t) * len(t[0])}] = {{"
                     + ", ".join(repr(float(v)) for row in t for v in row) + "};")
        lines.append("};")
    lines.append("")
    from dolfinx_eqlb_amd.lsolver.primal import load_table_exact, stiffness_table_exact
    lines.append("// reference stiffness of P_p: ST[m][i][j], S0 = int dX phi_i dX phi_j, S1 = int (dX phi_i dY phi_j + dY phi_i dX phi_j),")
    lines.append("// S2 = int dY phi_i dY phi_j (lsolver/primal.py, eqlb_primal_solve.hip)")
    lines.append("template <int P> struct Stiff;")
    for p in range(1, 5):
        t = stiffness_table_exact(p)
        n = len(t[0])
        lines.append(f"template <> struct Stiff<{p}> {{")
        lines.append(f"  static constexpr int ND = {n};")
        lines.append(f"  static constexpr double ST[{3 * n * n}] = {{"
                     + ", ".join(repr(float(v)) for m in t for row in m for v in row) + "};")
        lines.append("};")
    lines.append("")
    lines.append("// load of P_p against DG_d data: LD[i][n] = int phi_i chi_n, chi_n the DG_d nodal basis of rhs_dg")
    lines.append("template <int P, int D> struct Load;")
    for p in range(1, 5):
        for d in range(4):
            t = load_table_exact(p, d)
            lines.append(f"template <> struct Load<{p}, {d}> {{")
            lines.append(f"  static constexpr int NP = {len(t)}, ND = {len(t[0])};")
            lines.append(f"  static constexpr double LD[{len(t) * len(t[0])}] = {{"
                         + ", ".join(repr(float(v)) for row in t for v in row) + "};")
            lines.append("};")
    lines.append("")
    from dolfinx_eqlb_amd.lsolver.primal import cross_table_exact
    lines.append("// cross block of the reference stiffness of P_p: CR[i][j] = int dX phi_i dY phi_j; S1 == CR + CR^T exactly")
    lines.append("// (lsolver/primal.py, eqlb_primal_elasticity.hip)")
    lines.append("template <int P> struct Cross;")
    for p in range(1, 5):
        t = cross_table_exact(p)
        n = len(t)
        lines.append(f"template <> struct Cross<{p}> {{")
        lines.append(f"  static constexpr int ND = {n};")
        lines.append(f"  static constexpr double CR[{n * n}] = {{"
                     + ", ".join(repr(float(v)) for row in t for v in row) + "};")
        lines.append("};")
    lines.append("")
    from dolfinx_eqlb_amd.lsolver.primal import mass_table_exact, value_table_exact
    lines.append("// reference mass of P_p: MS[i][j] = int phi_i phi_j, the reaction term of eqlb_primal_* and eqlb_elasticity_*")
    lines.append("// (lsolver/primal.py: mass_table_exact)")
    lines.append("template <int P> struct Mass;")
    for p in range(1, 5):
        t = mass_table_exact(p)
        n = len(t)
        lines.append(f"template <> struct Mass<{p}> {{")
        lines.append(f"  static constexpr int ND = {n};")
        lines.append(f"  static constexpr double MS[{n * n}] = {{"
                     + ", ".join(repr(float(v)) for row in t for v in row) + "};")
        lines.append("};")
    lines.append("")
    lines.append("// L2 projection of P_p onto DG_d: PV[n][i] = DG_d nodal value n of the projection of phi_i (interpolation for")
    lines.append("// d >= p, MS<d>^-1 LD<p,d>^T below); eqlb_primal_value_dg (eqlb_primal_flux.hip)")
    lines.append("template <int P, int D> struct Value;")
    for (p, d) in PAIRS_PRIMAL:
        t = value_table_exact(p, d)
        lines.append(f"template <> struct Value<{p}, {d}> {{")
        lines.append(f"  static constexpr int NP = {len(t[0])}, ND = {len(t)};")
        lines.append(f"  static constexpr double PV[{len(t) * len(t[0])}] = {{"
                     + ", ".join(repr(float(v)) for row in t for v in row) + "};")
        lines.append("};")
    lines.append("")
    from dolfinx_eqlb_amd.mesh.transfer import flux_bc_table_exact
    lines.append("// facet DOFs of a flux boundary condition across one bisection level: FB[m][j][i], child DOF j from parent DOF i")
    lines.append("// for the maps m = (0,1), (1,0), (0,1/2), (1/2,1), (1/2,0), (1,1/2) of the facet parameter (mesh/transfer.py,")
    lines.append("// eqlb_bc_carry.hip)")
    lines.append("template <int K> struct FluxBcProlong;")
    for k in range(1, 5):
        t = flux_bc_table_exact(k)
        lines.append(f"template <> struct FluxBcProlong<{k}> {{")
        lines.append(f"  static constexpr double FB[{6 * k * k}] = {{"
                     + ", ".join(repr(float(v)) for m in t for row in m for v in row) + "};")
        lines.append("};")
    lines.append("")
    from dolfinx_eqlb_amd.lsolver.primal import facet_mass_table_exact
    lines.append("// mass of the trace of P_p on a facet of unit length: FM[i][j] = int_0^1 l_i l_j ds, l the equispaced 1-D Lagrange")
    lines.append("// basis in the local order (lower node id, higher node id, interior 0 ... p-2 from the lower to the higher node);")
    lines.append("// the Robin term of eqlb_primal_set_robin (lsolver/primal.py: facet_mass_table_exact)")
    lines.append("template <int P> struct FacetMass;")
    for p in range(1, 5):
        t = facet_mass_table_exact(p)
        n = len(t)
        lines.append(f"template <> struct FacetMass<{p}> {{")
        lines.append(f"  static constexpr int N = {n};")
        lines.append(f"  static constexpr double FM[{n * n}] = {{"
                     + ", ".join(repr(float(v)) for row in t for v in row) + "};")
        lines.append("};")
    lines.append("")
    lines.append("// reference facet normals of the RT functionals (e_raviart_thomas.py:82) and whether the")
    lines.append("// functional measures the outward flux")
    lines.append("static constexpr double NREF[3][2] = {{-1.0, -1.0}, {-1.0, 0.0}, {0.0, 1.0}};")
    lines.append("static constexpr bool NOUT[3] = {false, true, false};")
    lines.append("")
    lines.append("} // namespace eqlb_tables")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def emit_build(path):
    """The pairs of PAIRS_BUILD, behind the committed header (written by the build)."""
    lines = ["// GENERATED by tools/gen_tables.py --build at build time - do not edit, not in git.",
             "#pragma once", "", '#include "eqlb_tables_gen.h"', "", "namespace eqlb_tables {", ""]
    _emit_refs(lines, PAIRS_BUILD)
    lines.append("} // namespace eqlb_tables")
    tmp = path + ".tmp"
    with open(tmp, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    os.replace(tmp, path)  # a make interrupted mid-write leaves no truncated header behind


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    if len(sys.argv) == 3 and sys.argv[1] == "--build":
        emit_build(sys.argv[2])
        print("wrote", sys.argv[2])
    else:
        out = os.path.join(here, "..", "dolfinx_eqlb_amd", "csrc", "eqlb_tables_gen.h")
        emit(os.path.normpath(out))
        print("wrote", os.path.normpath(out))
