"""numpy statement of the weak-symmetry step as the banded kernel computes it for RT_3 / RT_4 on large patches
(test infrastructure; eqlb_se_weaksym_banded.hip, the companion of proto_stress_lanes.py for k >= 3).

Per patch the reference solves  [A 0 B0; 0 A B1; B0^T B1^T 0(+c)] [u0; u1; gamma] = [0; 0; Lc]
(se/PatchData.hpp:598-663).  Here the unknowns are ordered as a banded chain plus a border:

  * chain  [a_0 | x_1 | a_1 | x_2 | ...]: a_s the cell-bubble unknowns of cell s, x_f the k - 1 unknowns of
    facet f >= 1; border [d | x_0]: the patch-node unknown and facet 0.  A cell couples [x_s | a_s | x_{s+1}]
    and the border only: half bandwidth BW = 2 (k - 1) + (k - 1)(k - 2)/2 - 1, and the Cholesky factor keeps
    that profile (band + dense border rows);
  * B_k has at most four entries per row (the patch node and the ring points of the cells on either side of
    the row's facet), except the dense row of d;
  * S = sum_k Y_k^T Y_k with Y_k = L_k^-1 B_k (forward substitution only), C = M - S with the mean-value
    border M; C gamma = Lc by Gauss-Jordan with row pivoting and the rank-revealing threshold of the dense
    kernel (a column without pivot gets multiplier 0);
  * u_k = -A_k^-1 (B_k gamma), masked per stress row where that row has flux BCs.
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
from gen_tables import combo, tables_float  # noqa: E402

PIVOT_RTOL = 1e-11  # EQLB_WS_PIVOT_RTOL
_TABLES = {}


def tables(k):
    if k not in _TABLES:
        _TABLES[k] = tables_float(k, k - 1)
    return _TABLES[k]


def binom(n, r):
    v = 1
    for i in range(r):
        v = v * (n - i) // (i + 1)
    return v


def bcoef(j, i):
    return 0.0 if i > j else (1.0 if i % 2 == 0 else -1.0) * binom(j, i)


def element_data(mesh, k, fan, node, c0, c1):
    """Per-lane element quantities of the patch of `node`: Te [NH, NH], Be [2, NH, 3], Lce [3], Ce, the local
    facet / vertex ids; c0, c1 [ncells, k(k+2)]: the patch-local stress rows."""
    tab = tables(k)
    nrt, kb, nadd = k * (k + 2), k - 1, (k - 1) * (k - 2) // 2
    nh = 1 + 2 * kb + nadd
    n = int(fan["ncells"][node])
    cells = fan["cells"][node]
    fl, il, fcts = fan["fcts_local"][node], fan["inodes_local"][node], fan["fcts"][node]
    interior = cells[0] >= 0
    TE, VQ, V = tab["TE"], tab["VQ"], tab["V"]

    def perm(cell, fct):
        return mesh.facet_perm[cell, np.nonzero(mesh.cell_facets[cell] == fct)[0][0]]
    lanes = []
    for i in range(n):
        a = i + 1
        c = cells[a]
        fm, fp, ln = int(fl[2 * a - 1]), int(fl[2 * a]), int(il[a])
        x = mesh.x[mesh.cell_nodes[c], :2]
        J = np.stack([x[1] - x[0], x[2] - x[0]], axis=1)
        detJ = np.linalg.det(J)
        sgn = 1.0 if detJ > 0 else -1.0
        rev_m = False
        if interior or a > 1:
            rev_m = bool(perm(cells[a - 1], fcts[a - 1]) != perm(c, fcts[a - 1]))
        ci = combo(fm, fp, int(rev_m))
        g = J.T @ J / abs(detJ)
        te = g[0, 0] * TE[ci][0] + g[0, 1] * TE[ci][1] + g[1, 1] * TE[ci][2]
        Te = np.zeros((nh, nh))
        for h in range(nh):
            for gg in range(h + 1):
                Te[h, gg] = Te[gg, h] = te[h * (h + 1) // 2 + gg]
        v0, v1 = VQ[ci][0], VQ[ci][1]  # [NH, 3]
        Be = np.stack([J[1, 0] * v0 + J[1, 1] * v1, -(J[0, 0] * v0 + J[0, 1] * v1)])
        w0 = c0[c] * J[1, 0] - c1[c] * J[0, 0]
        w1 = c0[c] * J[1, 1] - c1[c] * J[0, 1]
        Lce = -sgn * (V[:, :, 0] @ w0 + V[:, :, 1] @ w1)
        lanes.append(dict(c=c, fm=fm, fp=fp, ln=ln, Te=Te, Be=Be, Lce=Lce, Ce=abs(detJ) / 6.0, rev_m=rev_m,
                          sgn=sgn, pf_m=sgn if fm == 1 else -sgn, pf_p=sgn if fp == 1 else -sgn))
    assert nrt == c0.shape[1]
    return n, interior, lanes


class BandedFactor:
    """Cholesky factor of the patch matrix in chain + border order: band [nch, BW + 1] (band[i, d] = L[i, i - d]),
    border rows bord [NBD, dim] (border-border part in the columns nch ...), dinv = 1 / L_ii."""

    def __init__(self, A, nch, bw):
        dim = A.shape[0]
        self.nch, self.bw, self.nbd = nch, bw, dim - nch
        band = np.zeros((nch, bw + 1))
        for i in range(nch):
            for d in range(min(bw, i) + 1):
                band[i, d] = A[i, i - d]
        assert all(A[i, j] == 0.0 for i in range(nch) for j in range(i - bw)), "outside the band"
        bord = A[nch:, :].copy()
        dinv = np.zeros(dim)
        ok = True
        # right-looking: column j updates the BW band rows below it and the border rows
        for j in range(nch):
            ajj = band[j, 0]
            ok &= bool(ajj > 0.0 and np.isfinite(ajj))
            ljj = np.sqrt(ajj if ajj > 0.0 else 1.0)
            band[j, 0], dinv[j] = ljj, 1.0 / ljj
            rows = [i for i in range(j + 1, min(j + bw, nch - 1) + 1)]
            for i in rows:
                band[i, i - j] /= ljj
            bord[:, j] /= ljj
            for ia in rows:
                for ib in rows:
                    if ib <= ia:
                        band[ia, ia - ib] -= band[ia, ia - j] * band[ib, ib - j]
            for b in range(self.nbd):
                for ib in rows:
                    bord[b, ib] -= bord[b, j] * band[ib, ib - j]
                for bb in range(b + 1):
                    bord[b, nch + bb] -= bord[b, j] * bord[bb, j]
        for j in range(self.nbd):
            ajj = bord[j, nch + j]
            ok &= bool(ajj > 0.0 and np.isfinite(ajj))
            ljj = np.sqrt(ajj if ajj > 0.0 else 1.0)
            bord[j, nch + j], dinv[nch + j] = ljj, 1.0 / ljj
            for i in range(j + 1, self.nbd):
                bord[i, nch + j] /= ljj
            for i in range(j + 1, self.nbd):
                for kk in range(j + 1, i + 1):
                    bord[i, nch + kk] -= bord[i, nch + j] * bord[kk, nch + j]
        self.band, self.bord, self.dinv, self.ok = band, bord, dinv, ok

    def forward(self, b):
        """L^-1 b (columns of b)."""
        nch, bw = self.nch, self.bw
        y = np.array(b, dtype=float, copy=True)
        for i in range(nch):
            for d in range(1, min(bw, i) + 1):
                y[i] -= self.band[i, d] * y[i - d]
            y[i] *= self.dinv[i]
        for b_ in range(self.nbd):
            y[nch + b_] -= self.bord[b_, :nch + b_] @ y[:nch + b_]
            y[nch + b_] *= self.dinv[nch + b_]
        return y

    def backward(self, y):
        """L^-T y."""
        nch, bw = self.nch, self.bw
        x = np.array(y, dtype=float, copy=True)
        for b_ in reversed(range(self.nbd)):
            for q in range(b_ + 1, self.nbd):
                x[nch + b_] -= self.bord[q, nch + b_] * x[nch + q]
            x[nch + b_] *= self.dinv[nch + b_]
        for i in reversed(range(nch)):
            for d in range(1, bw + 1):
                if i + d < nch:
                    x[i] -= self.band[i + d, d] * x[i + d]
            x[i] -= self.bord[:, i] @ x[nch:]
            x[i] *= self.dinv[i]
        return x


def gauss_jordan(C, R):
    """C gamma = R by Gauss-Jordan with row pivoting (first row of largest modulus); a column whose pivot is not
    above PIVOT_RTOL * max|C| gets multiplier 0.  Returns (gamma, ok)."""
    C, R = C.copy(), R.copy()
    m = C.shape[0]
    ok = bool(np.isfinite(C).all())
    ptol = PIVOT_RTOL * np.abs(C).max()
    nr, pcol = 0, [-1] * m
    for c in range(m):
        if nr == m:
            continue
        piv = nr + int(np.argmax(np.abs(C[nr:, c])))
        if not np.abs(C[piv, c]) > ptol:
            continue
        C[[nr, piv]], R[[nr, piv]] = C[[piv, nr]], R[[piv, nr]]
        for r in range(nr + 1, m):
            f = C[r, c] / C[nr, c]
            C[r, c:] -= f * C[nr, c:]
            R[r] -= f * R[nr]
        pcol[c], nr = nr, nr + 1
    g = np.zeros(m)
    for c in reversed(range(m)):
        if pcol[c] >= 0:
            r = pcol[c]
            g[c] = (R[r] - C[r, c + 1:] @ g[c + 1:]) / C[r, c]
    return g, ok and bool(np.isfinite(g).all())


def weaksym_blocks(k, n, interior, lanes, bc0=(False, False), bcn=(False, False)):
    """Corrections ul [2, n, NH] (local unknowns [d | um | up | ua] of every lane, per stress row); bc0 / bcn:
    flux BCs of the first / last facet of a boundary patch per stress row.  Returns (ul, ok)."""
    kb, nadd = k - 1, (k - 1) * (k - 2) // 2
    nh = 1 + 2 * kb + nadd
    nbd, bw = 1 + kb, 2 * kb + nadd - 1
    nf = n if interior else n + 1
    dim = 1 + kb * nf + nadd * n
    nch, npnt = dim - nbd, nf + 1
    requires_bcs = any(bc0) or any(bcn)
    row_dual = [not interior and bc0[r] and bcn[r] for r in range(2)]
    meanvalue = interior or (row_dual[0] and row_dual[1])
    dim_c = npnt + 1 if meanvalue else npnt

    def pos_facet(f, m):
        return nch + 1 + m if f == 0 else (f - 1) * (kb + nadd) + nadd + m

    # numbering of every lane: positions of the local unknowns, multiplier DOFs of the local vertices
    pos, pj = [], []
    for s, L in enumerate(lanes):
        fi_p = ((s + 1) % n) if interior else s + 1
        p = [nch] + [pos_facet(s, j) for j in range(kb)] + [pos_facet(fi_p, j) for j in range(kb)]
        p += [s * (kb + nadd) + q for q in range(nadd)]
        pos.append(p)
        v_ea, v_eam1 = 3 - L["fp"] - L["ln"], 3 - L["fm"] - L["ln"]
        p_ea = s + 1 if interior else (nf if s + 1 == n else s + 1)
        p_eam1 = (n if s == 0 else s) if interior else (nf - 1 if s == 0 else s)
        pj.append([0 if j == L["ln"] else (p_ea if j == v_ea else (p_eam1 if j == v_eam1 else 0))
                   for j in range(3)])

    def fixed(r, s, h):
        if not requires_bcs:
            return False
        if h == 0:
            return bc0[r] or bcn[r]
        if h <= kb:
            return bc0[r] and s == 0
        if h <= 2 * kb:
            return bcn[r] and s == n - 1
        return False

    # B_k (dense here; the kernel keeps it compressed), C = M - S, R = Lc
    B = np.zeros((2, dim, npnt))
    C = np.zeros((dim_c, dim_c))
    R = np.zeros(dim_c)
    for s, L in enumerate(lanes):
        for r in range(2):
            for h in range(nh):
                if not fixed(r, s, h):
                    for j in range(3):
                        B[r, pos[s][h], pj[s][j]] += L["Be"][r, h, j]
        for j in range(3):
            R[pj[s][j]] += L["Lce"][j]
            if meanvalue:
                C[pj[s][j], npnt] += L["Ce"]
                C[npnt, pj[s][j]] += L["Ce"]
    assert all(np.count_nonzero(B[r, q]) <= 4 for r in range(2) for q in range(dim) if q != nch)

    def matrix(r):
        A = np.zeros((dim, dim))
        for s, L in enumerate(lanes):
            for h in range(nh):
                for g in range(nh):
                    if not fixed(r, s, h) and not fixed(r, s, g):
                        A[pos[s][h], pos[s][g]] += L["Te"][h, g]
        for s in range(n):
            for h in range(nh):
                if fixed(r, s, h):
                    A[pos[s][h], pos[s][h]] = 1.0
        return A

    factors = [BandedFactor(matrix(0), nch, bw)]
    factors.append(BandedFactor(matrix(1), nch, bw) if requires_bcs else factors[0])
    ok = factors[0].ok and factors[1].ok
    for r in range(2):
        Y = factors[r].forward(B[r])
        C[:npnt, :npnt] -= Y.T @ Y
    gam, ok_lu = gauss_jordan(C, R)
    ul = np.zeros((2, n, nh))
    for r in range(2):
        w = factors[r].backward(factors[r].forward(-(B[r] @ gam[:npnt])))
        for s in range(n):
            ul[r, s] = w[pos[s]]
    return ul, ok and ok_lu


def stress_correction(mesh, k, fan, node, c0, c1, bc0=(False, False), bcn=(False, False)):
    """Rows 0 / 1 of the weak-symmetry correction of the patch of `node` in RT coefficients
    [2, ncells, k(k+2)] (se/solve_patch_weaksym.hpp:189-232), from the patch-local rows c0, c1."""
    kb, nadd = k - 1, (k - 1) * (k - 2) // 2
    ndiv = k * (k + 1) // 2 - 1
    n, interior, lanes = element_data(mesh, k, fan, node, c0, c1)
    ul, ok = weaksym_blocks(k, n, interior, lanes, bc0, bcn)
    assert ok
    out = np.zeros((2, mesh.ncells, k * (k + 2)))
    Bm = np.array([[bcoef(j, c) for c in range(k)] for j in range(k)])
    for r in range(2):
        for i, L in enumerate(lanes):
            u = ul[r, i]
            s = -((Bm if L["rev_m"] else np.eye(k)) @ u[:k])
            yp = np.concatenate([[u[0]], u[1 + kb:1 + 2 * kb]])
            out[r, L["c"], L["fm"] * k:(L["fm"] + 1) * k] += L["pf_m"] * s
            out[r, L["c"], L["fp"] * k:(L["fp"] + 1) * k] += L["pf_p"] * yp
            out[r, L["c"], 3 * k + ndiv:3 * k + ndiv + nadd] += L["sgn"] * u[1 + 2 * kb:]
    return out
