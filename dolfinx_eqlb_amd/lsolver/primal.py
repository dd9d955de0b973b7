"""The P_p Poisson problem -div(kappa grad u) = f on the handle's own space - the statement of the rule.

The adaptive demos of the reference solve the primal problem with PETSc (demo/poisson_adaptive/demo_lshape.py,
demo_discont-coeff.py, demo/poisson/demo_reconstruction.py).  This file defines, in numpy, what the device path
(eqlb_primal_* of include/eqlb.h, csrc/eqlb_primal_solve.hip) computes; the device reproduces the operator, the load,
the diagonal and the residual bit for bit.

  space     the numbering of mesh/transfer.py: lagrange_dofmap, equispaced P_p in Basix order, 1 <= p <= 4.  The owner
            of a DOF follows from its index: d < nnodes is a vertex DOF, then nfacets (p-1) facet DOFs, then the
            cell-interior DOFs
  tables    Stiff<p> [3][nd_p][nd_p]: S0 = int dX phi_i dX phi_j, S1 = int (dX phi_i dY phi_j + dY phi_i dX phi_j),
            S2 = int dY phi_i dY phi_j on the reference triangle; Load<p,d> [nd_p][nd_d]: int phi_i chi_n with chi_n the
            DG_d nodal basis of rhs_dg.  Exact Fractions, each rounded once to double
  geometry  J = (x1 - x0 | x2 - x0) (the handle's cellJ), det = J00 J11 - J01 J10, idet = 1 / det,
            K00 = J11 idet, K01 = -J01 idet, K10 = -J10 idet, K11 = J00 idet,
            C00 = K00 K00 + K01 K01, C01 = K00 K10 + K01 K11, C11 = K10 K10 + K11 K11, w = kappa_c |det|
  cell      t_m[i] = sum_j S_m[i][j] u[dof(c, j)], m = 0, 1, 2: every product rounded on its own, added in ascending j;
            y_loc[c][i] = w ((C00 t_0[i] + C01 t_1[i]) + C11 t_2[i]); every operation rounded on its own (no fused
            multiply-add)
  owner sum y[d] = the y_loc entries of DOF d, added from the first cell on: a vertex DOF takes the cells in the order
            of the node -> cell table, a facet DOF those of the facet -> cell table, an interior DOF has its one cell
  load      per cell |det| (sum_n Load[i][n] rhs_dg[c][n]) (ascending n), through the same owner sum, + b_extra[d]
  diagonal  w ((C00 S0[i][i] + C01 S1[i][i]) + C11 S2[i][i]) through the same owner sum
  residual  r = b - A u, 0 on the rows where `fixed` is set

THE REACTION TERM (set_reaction; eqlb_primal_set_reaction / eqlb_elasticity_set_reaction): the operator becomes
-div(kappa grad u) + c u, or -div(2 eps(u) + pi_1 div(u) I) + c u, with c_T >= 0 per cell, one scalar or a cell-wise
array in the pi_1 / cell_pi1 convention.  New table Mass<p> [nd_p][nd_p] = int phi_i phi_j on the reference triangle,
exact Fractions, each rounded once.  Per cell
  wm        = c_T |det|
  m^s[i]    = sum_j Mass[i][j] u_s[j], ascending j, every product rounded on its own, no fused multiply-add
  Poisson   : y_loc[c][i]    = (the value of the rule above) + wm m[i]
  elasticity: y_loc[c][i][r] = (the value of the rule below) + wm m^r[i]
  diagonal  : (the value above / below) + wm Mass[i][i], for both units and both components
one product and one addition on top of the value formed without the term; everything before that addition, the load,
the owner sum, the mask, the residual, the reference norm and pcg are unchanged.  c = 0 without an array switches the
term off: the operator is then the one of a fresh object, bit for bit.

THE DIFFUSION TENSOR (PoissonOperator.set_diffusion; eqlb_primal_set_diffusion): the operator becomes
-div(kappa D grad u) [+ c u] with a symmetric positive definite D_T per cell, cell_D [ncells, 3] = (d00, d01, d11).
Per cell, with K[X][d] as above and D[0][1] = D[1][0] = d01,
  T[X][b]   = K[X][0] D[0][b] + K[X][1] D[1][b]
  C_XY      = T[X][0] K[Y][0] + T[X][1] K[Y][1]        for XY = 00, 01, 11
every product and every sum rounded on its own; C00, C01, C11 and w = kappa |det| then enter the cell rule, the diagonal
and the reaction variant exactly as above.  The load is unchanged.  D = I gives the values of an operator without the
term (signs of zero aside); None switches the term off: the operator is then the one of a fresh object, bit for bit.
A cell with a value that is not finite, or where d00 > 0 and d00 d11 - d01^2 > 0 do not both hold, is refused by name.
D is DG_0 data with three components: it crosses a refinement through Refinement.prolong_dg(0, cell_D.ravel(), bs=3).
diffusion_oscillation_weight gives the factor 1 / sqrt(lambda_min(kappa_T D_T)) of the data oscillation.

THE SHEAR MODULUS (ElasticityOperator.set_shear; eqlb_elasticity_set_shear): the operator becomes
-div(mu (2 eps(u) + pi_1 div(u) I)) [+ c u] with mu_T > 0 per cell, one scalar or a cell-wise array in the pi_1 /
cell_pi1 convention.  Per cell, with v the value of the elasticity rule below (before any reaction term),
  y_loc[c][i][r] = mu_T v;   with a reaction term  y_loc[c][i][r] = (mu_T v) + wm m^r[i]
one product on top of the value formed without the term, no fused multiply-add; the reaction term is not scaled by
mu.  The diagonal follows the same rule, the load is unchanged.  mu = 1 without an array switches the term off: the
operator is then the one of a fresh object, bit for bit; a uniform power of two scales every bit pattern exactly.

THE ROBIN TERM (PoissonOperator.set_robin; eqlb_primal_set_robin, Poisson only): on the listed boundary facets
-(kappa D grad u) . n = alpha (u - u_ext) with alpha_f >= 0 per facet, one scalar or a list-wise array.  The operator gains
the boundary mass int_E alpha u v; the datum int_E alpha u_ext v is a load (robin_load).  New table FacetMass<p> [p+1][p+1]
= int_0^1 l_i l_j ds, l the equispaced 1-D Lagrange basis of degree p in the local order (lower node id, higher node id,
interior 0 ... p-2 from the lower to the higher node) - the order of the global DOFs lo, hi, nnodes + f (p-1) + j of a
facet, so no cell is needed to find a facet's rows.  Exact Fractions, each rounded once.  Per listed facet
  w_f       = alpha_f |E_f|, |E| = sqrt(dx dx + dy dy), dx = x[n1] - x[n0] from facet_nodes, every operation rounded on its
              own; formed once at set_robin and kept (robin_weights)
  t_f[i]    = w_f (sum_j FacetMass[i][j] u[dof_j]), ascending j, every product rounded on its own, no fused multiply-add
  row d     : the owner sum as above, then the t_f[i] of the Robin facets that hold d, in ascending facet id, each by one
              addition; b_extra, the mask, r = b - v and the inner products behind that are unchanged.  The lifting (u^)
              reads the free rows of u as 0 in the facet term too
  diagonal  : the owner sum, then + w_f FacetMass[i][i] in the same place
  matrix    : + w_f FacetMass[i][j] on entry (d, d') after the cell sums, facets ascending; the pattern holds every pair
An empty list switches the term off: the operator is then the one of a fresh object, bit for bit; alpha_f = 0 on a listed
facet is allowed.  Refused by facet, before anything changes: a listed facet that is no boundary facet, a facet listed
twice, an alpha that is negative, NaN or infinite.  With some alpha_f > 0 the operator is positive definite without a
fixed DOF, and pcg no longer asks for one.  The owner sum of the load and of the restriction of a hierarchy stays plain.
robin_flux states eqlb_primal_robin_flux, alpha (u_h - u_ext) at points of the listed facets: the flux condition
sigma_eq . n of the equilibrator that the discrete solution implies.

THE SPRING TERM (ElasticityOperator.set_springs; eqlb_elasticity_set_springs): the counterpart on the blocked space,
sigma(u) n = -K_f (u - u_ext) on the listed boundary facets with K_f a symmetric positive semidefinite 2 x 2 tensor per
facet in global axes, facet_k [nlist][3] = (k00, k01, k11), the layout of cell_D - an elastic foundation, a compliant
support, a penalised sliding (K = kn n x n, spring_tensor) or clamped side.  The operator gains int_E v^T K u; the datum
int_E v^T K u_ext is a load (spring_load).  FacetMass<p> and the local order of a facet are those of the Robin term.
  Kw_f      = (|E_f| k00, |E_f| k01, |E_f| k11), |E_f| of facet_lengths, one product per entry; formed once at
              set_springs and kept (spring_weights)
  m[i][s]   = sum_j FacetMass[i][j] u[2 dof_j + s], ascending j, every product rounded on its own
  t_f[i][r] = Kw[r][0] m[i][0] + Kw[r][1] m[i][1]: two products and one addition, no fused multiply-add
  row 2d+r  : the owner sum, then the t_f[i][r] of the spring facets that hold d, in ascending facet id, each by one
              addition; everything behind that unchanged, the lifting reads a free row 2 dof_j + s as 0 here too
  diagonal  : the owner sum, then + Kw[r][r] FacetMass[i][i] in the same place
  matrix    : + Kw[r][s] FacetMass[i][j] on entry (2 d_i + r, 2 d_j + s) after the cell sums, facets ascending; the
              blocked pattern holds the full 2 x 2 block of every pair of DOFs of a cell, hence of a facet
Refused by facet in list order, before anything changes (spring_list): no boundary facet, listed twice, an entry that
is not finite, k00 < 0, k11 < 0, k01 k01 > (k00 k11) (1 + 2^-49) - the allowance lets a rank-one tensor formed in
floating point as kn n_a n_b pass.  With some listed facet of |E_f| > 0 and K_f positive definite, k00 > 0 and
k01 k01 < (k00 k11) (1 - 2^-49), no rigid motion is left and pcg asks for no Dirichlet DOF in either component
(spring_positive); a list of rank-one tensors leaves the per-component rule as it was.  spring_flux states
eqlb_elasticity_spring_flux, K (u_h - u_ext) at points of the listed facets: row r is the flux condition of stress row r.

value_dg states eqlb_primal_value_dg, the piece that turns c u_h into the right-hand side the equilibrator needs
(rhs = Pi_d f - c_T Pi_d u_h): out[r][c][n] = coeff[c] sum_i PV<p,d>[n][i] u[r][cell_dofs[c][i]], ascending i, every
product rounded on its own, with PV<p,d> [nd_d][nd_p] the DG_d nodal values of the L2 projection of phi_i onto P_d:
interpolation for d >= p, Mass<d>^-1 Load<p,d>^T in Fractions below.

Every statement can return the sum of the absolute values of its terms (return_abs), so that a test bounds the
comparison with an independently rounded computation by terms * 2^-53 * abs-sum.

pcg() states the Jacobi-preconditioned CG of eqlb_primal_solve with np.sum for the inner products: the reference for
iteration counts and for the host tests (the device reduces in another order, so its iterates differ in the last bits).

ElasticityOperator states the same for -div(2 eps(u) + pi_1 div(u) I) = f on [P_p]^2 (eqlb_elasticity_* of
include/eqlb.h, csrc/eqlb_primal_elasticity.hip), the primal solve of demo/elasticity_adaptive/demo_cook.py, in the
non-dimensional form and with the pi_1 / cell_pi1 convention of eqlb_primal_stress_dg:

  layout    the scalar numbering of lagrange_dofmap, blocked: u[2 dof + r]
  tables    S0, S2 of Stiff<p> and Cross<p> [nd_p][nd_p] = int dX phi_i dY phi_j: M_00 = S0, M_01 = Cross,
            M_10 = Cross^T, M_11 = S2 (S1 == Cross + Cross^T exactly)
  geometry  K as above, K[X][d]; Q[a][b][X][Y] = K[X][a] K[Y][b]
  cell      g_XY^s[i] = sum_j M_XY[i][j] u_s[j], u_s[j] = u[2 dof(c, j) + s], ascending j, products rounded one by one;
            D_ab^s[i] = (Q[a][b][0][0] g_00^s[i] + Q[a][b][0][1] g_01^s[i])
                      + (Q[a][b][1][0] g_10^s[i] + Q[a][b][1][1] g_11^s[i])          ( = int d_a phi_i d_b u_s )
            y_loc[c][i][0] = |det| (((D_00^0 + D_11^0) + (D_00^0 + D_10^1)) + pi_c (D_00^0 + D_01^1))
            y_loc[c][i][1] = |det| (((D_00^1 + D_11^1) + (D_01^0 + D_11^1)) + pi_c (D_10^0 + D_11^1))
            that is |det| ((D_00^r + D_11^r) + sum_s D_sr^s + pi_c sum_s D_rs^s); no fused multiply-add
  owner sum as above, per (dof, r)
  load      per cell and component |det| (sum_n Load[i][n] rhs_dg[r][c][n]) through the owner sum, + b_extra[2 d + r]
  diagonal  g_XY = M_XY[i][i], D_ab as above, |det| (((D_00 + D_11) + D_rr) + pi_c D_rr) through the owner sum

THE ASSEMBLED MATRIX (PoissonOperator.matrix, ElasticityOperator.matrix, csr_apply; eqlb_primal_matrix_*,
eqlb_elasticity_matrix_*, eqlb_csr_apply of include/eqlb.h, csrc/eqlb_primal_matrix.hip): the operator as CSR,
(indptr int64 [n + 1], indices int32 [nnz], values float64 [nnz]) with n = bs ndofs rows in the numbering of the vectors
(elasticity blocked, 2 dof + r); the device reproduces the three arrays bit for bit.
  pattern   row bs d + r holds every column bs d' + s (all s) such that d and d' lie in a common cell; columns ascending,
            each once; an entry whose value happens to be 0.0 stays.  It depends on the mesh and p alone
  cell entry, Poisson      the rule of `diagonal` with the table entry [i][j] in the place of [i][i]:
            w ((C00 S0[i][j] + C01 S1[i][j]) + C11 S2[i][j]), then + wm Mass[i][j] with a reaction term; C from K, or from
            K D K^T with set_diffusion, as above
  cell entry, elasticity   D_ab of `diagonal` with g_XY = M_XY[i][j] (g_01 = Cross[i][j], g_10 = Cross[j][i]); entry
            ((i, r), (j, s)) = |det| (((D_00 + D_11) + D_rr) + pi_c D_rr)   for r == s
                             = |det| (D_sr + pi_c D_rs)                      for r != s
            the terms of y_loc[c][i][r] that carry u_s[j], in their order, absent terms dropped (not added as zeros); with
            set_shear times mu_T; with set_reaction + wm Mass[i][j] for r == s only, after the shear product
  sum       over the cells of the row's DOF that also hold the column's DOF, from the first on, in the order of the slot
            list of the row's DOF (the owner sum).  The diagonal of the raw matrix therefore has the bits of diagonal()
  eliminate False: the raw operator, what apply(u, masked=False) applies.  True: P A P + (I - P): an entry with a fixed
            row or column is 0.0 off the diagonal and 1.0 on it, and stays in the pattern.  The lifting of inhomogeneous
            Dirichlet values is what residual(b, u_D) returns
  csr_apply y[row] = the sum over the positions of the row in ascending order, the first product starts it, then
            s = s + v x, product and sum rounded on their own; an empty row gives 0.0
every operation rounded on its own, no fused multiply-add.
"""

from fractions import Fraction
from functools import lru_cache

import numpy as np

from ..elmtlib import polynomials as P
from ..elmtlib.lagrange import Lagrange
from ..mesh.transfer import lagrange_dofmap, nd_of


@lru_cache(maxsize=None)
def stiffness_table_exact(p):
    """S [3][nd_p][nd_p] Fractions."""
    if p < 1 or p > 4:
        raise ValueError(f"stiffness_table: p = {p} outside 1 ... 4")
    basis = Lagrange(p).basis
    dx, dy = [P.ddx(b) for b in basis], [P.ddy(b) for b in basis]
    n = len(basis)
    integ = P.integrate_triangle
    S0 = tuple(tuple(integ(P.mul(dx[i], dx[j])) for j in range(n)) for i in range(n))
    S1 = tuple(tuple(integ(P.mul(dx[i], dy[j])) + integ(P.mul(dy[i], dx[j])) for j in range(n)) for i in range(n))
    S2 = tuple(tuple(integ(P.mul(dy[i], dy[j])) for j in range(n)) for i in range(n))
    return (S0, S1, S2)


@lru_cache(maxsize=None)
def load_table_exact(p, d):
    """Load [nd_p][nd_d] Fractions."""
    if p < 1 or p > 4 or d < 0 or d > 3:
        raise ValueError(f"load_table: p = {p}, d = {d} outside 1 ... 4, 0 ... 3")
    phi, chi = Lagrange(p).basis, Lagrange(d).basis
    return tuple(tuple(P.integrate_triangle(P.mul(a, b)) for b in chi) for a in phi)


@lru_cache(maxsize=None)
def cross_table_exact(p):
    """Cross [nd_p][nd_p] Fractions: int dX phi_i dY phi_j on the reference triangle.  S1 == Cross + Cross^T exactly."""
    if p < 1 or p > 4:
        raise ValueError(f"cross_table: p = {p} outside 1 ... 4")
    basis = Lagrange(p).basis
    dx, dy = [P.ddx(b) for b in basis], [P.ddy(b) for b in basis]
    n = len(basis)
    return tuple(tuple(P.integrate_triangle(P.mul(dx[i], dy[j])) for j in range(n)) for i in range(n))


@lru_cache(maxsize=None)
def mass_table_exact(p):
    """Mass [nd_p][nd_p] Fractions: int phi_i phi_j on the reference triangle, 0 <= p <= 4 (the device knows p >= 1;
    p = 0 serves the projection identity of value_table_exact)."""
    if p < 0 or p > 4:
        raise ValueError(f"mass_table_exact: p = {p} outside 0 ... 4")
    basis = Lagrange(p).basis
    n = len(basis)
    return tuple(tuple(P.integrate_triangle(P.mul(basis[i], basis[j])) for j in range(n)) for i in range(n))


def mass_table(p):
    """The table [nd_p, nd_p] as doubles, each entry rounded once."""
    if p < 1:
        raise ValueError(f"mass_table: p = {p} outside 1 ... 4")
    return np.array([[float(v) for v in row] for row in mass_table_exact(p)])


@lru_cache(maxsize=None)
def value_table_exact(p, d):
    """PV [nd_d][nd_p] Fractions: DG_d nodal value n of the L2 projection of phi_i (the basis of P_p) onto P_d.  For
    d >= p that is the value of phi_i at node n of DG_d; below it is Mass<d>^-1 Load<p,d>^T, whose |det J| cancels on an
    affine cell."""
    if p < 1 or p > 4 or d < 0 or d > 3:
        raise ValueError(f"value_table: p = {p}, d = {d} outside 1 ... 4, 0 ... 3")
    phi, dg = Lagrange(p).basis, Lagrange(d)
    if d >= p:
        def at(q, x, y):
            return sum((c * x ** a * y ** b for (a, b), c in q.items()), Fraction(0))
        return tuple(tuple(at(q, *dg.nodes[n]) for q in phi) for n in range(dg.ndofs))
    load = load_table_exact(p, d)
    rhs = [[load[i][n] for i in range(len(phi))] for n in range(dg.ndofs)]
    return tuple(tuple(row) for row in P.solve_exact([list(r) for r in mass_table_exact(d)], rhs))


def value_table(p, d):
    """The table [nd_d, nd_p] as doubles, each entry rounded once."""
    return np.array([[float(v) for v in row] for row in value_table_exact(p, d)])


def _lagrange_1d_exact(p):
    """Coefficient lists (ascending powers, Fractions) of the equispaced 1-D Lagrange basis of degree p on [0, 1] in the
    local order of a facet: the node at 0, the node at 1, then the interior nodes 1/p ... (p-1)/p."""
    nodes = [Fraction(0), Fraction(1)] + [Fraction(j, p) for j in range(1, p)]
    out = []
    for i, xi in enumerate(nodes):
        c = [Fraction(1)]
        for k, xk in enumerate(nodes):
            if k != i:
                den = xi - xk
                c = [(c[n - 1] if n else Fraction(0)) / den - (c[n] * xk / den if n < len(c) else Fraction(0))
                     for n in range(len(c) + 1)]
        out.append(tuple(c))
    return tuple(out)


@lru_cache(maxsize=None)
def facet_mass_table_exact(p):
    """FacetMass [p+1][p+1] Fractions: int_0^1 l_i l_j ds in the local order of a facet (the head of this file)."""
    if p < 1 or p > 4:
        raise ValueError(f"facet_mass_table: p = {p} outside 1 ... 4")
    L = _lagrange_1d_exact(p)

    def integ(a, b):
        return sum((ca * cb / (m + n + 1) for m, ca in enumerate(a) for n, cb in enumerate(b)), Fraction(0))
    return tuple(tuple(integ(a, b) for b in L) for a in L)


def facet_mass_table(p):
    """The table [p+1, p+1] as doubles, each entry rounded once."""
    return np.array([[float(v) for v in row] for row in facet_mass_table_exact(p)])


def facet_basis(p, s):
    """l_i(s) [nq, p+1] of the equispaced 1-D Lagrange basis in the local order of a facet: the product over the other
    nodes k, in that order, of (s - x_k) / (x_i - x_k) with x = (0, 1, 1/p ... (p-1)/p) formed as j / p in doubles; the
    first factor starts the product, every operation rounded on its own (the rule of eqlb_primal_robin_flux)."""
    s = np.asarray(s, dtype=np.float64).ravel()
    x = [0.0, 1.0] + [j / float(p) for j in range(1, p)]
    out = np.empty((s.size, p + 1))
    for i in range(p + 1):
        v = None
        for k in range(p + 1):
            if k != i:
                fac = (s - x[k]) / (x[i] - x[k])
                v = fac if v is None else v * fac
        out[:, i] = v
    return out


def robin_list(who, mesh, facets, alpha=1.0, facet_alpha=None):
    """(facets int64 [n], alpha [n]) of set_robin in the order given, or (None, None) for an empty list.  Refused by
    facet: one that is no boundary facet of the mesh, one listed twice, an alpha that is negative, NaN or infinite."""
    f = np.asarray([] if facets is None else facets, dtype=np.int64).ravel()
    if facet_alpha is None:
        a = float(alpha)
        if not (a >= 0.0 and np.isfinite(a)):
            raise ValueError(f"{who}: alpha = {a} is negative, NaN or infinite")
        al = np.full(f.size, a)
    else:
        al = np.array(facet_alpha, dtype=np.float64).ravel()
        if al.size != f.size:
            raise ValueError(f"{who}: facet_alpha [nlist] expected")
    fco = mesh.facet_cells_offsets
    seen = set()
    for i, v in enumerate(f):
        v = int(v)
        if v < 0 or v >= mesh.nfacets or fco[v + 1] - fco[v] != 1:
            raise ValueError(f"{who}: facets[{i}] = {v} is no boundary facet of the mesh")
        if v in seen:
            raise ValueError(f"{who}: facets[{i}] = {v} is listed twice")
        seen.add(v)
        if not (al[i] >= 0.0 and np.isfinite(al[i])):
            raise ValueError(f"{who}: facet_alpha[{i}] = {al[i]} is negative, NaN or infinite")
    return (None, None) if f.size == 0 else (f, al)


def facet_lengths(mesh, facets):
    """|E_f| = sqrt(dx dx + dy dy), dx = x[n1] - x[n0] from facet_nodes, every operation rounded on its own."""
    fn = mesh.facet_nodes[np.asarray(facets, dtype=np.int64)]
    dx = mesh.x[fn[:, 1], 0] - mesh.x[fn[:, 0], 0]
    dy = mesh.x[fn[:, 1], 1] - mesh.x[fn[:, 0], 1]
    return np.sqrt(dx * dx + dy * dy)


def facet_dofs(mesh, p, facets):
    """[n, p+1] int64: the rows of a facet in its local order: lower node id, higher node id, nnodes + f (p-1) + j."""
    f = np.asarray(facets, dtype=np.int64).ravel()
    fn = mesh.facet_nodes[f].astype(np.int64)
    cols = [fn.min(axis=1), fn.max(axis=1)] + [mesh.nnodes + f * (p - 1) + j for j in range(p - 1)]
    return np.stack(cols, axis=1)


def robin_load(mesh, p, facets, alpha, u_ext, quadrature_degree=None):
    """b_extra [ndofs] = int_E alpha u_ext phi_i over the listed boundary facets, on the host: BY DEFINITION
    neumann_load with g = -alpha u_ext, bit for bit that call.  alpha: a scalar or one value per listed facet; u_ext a
    callable (x, y) -> values."""
    from types import SimpleNamespace
    f = np.asarray(facets, dtype=np.int64).ravel()
    al = np.broadcast_to(np.asarray(alpha, dtype=np.float64), f.shape)
    bcs = [SimpleNamespace(facets=[int(v)], scalar=True,
                           value=(lambda x, y, a=float(a): -a * np.asarray(u_ext(x, y), dtype=np.float64)))
           for v, a in zip(f, al)]
    return neumann_load(mesh, p, bcs, quadrature_degree)


def robin_flux(mesh, p, facets, facet_alpha, u, s, u_ext=None):
    """The statement of eqlb_primal_robin_flux: out [n, nq] = alpha_i (u_h(x_q) - u_ext[i][q]) on the listed facets at
    the facet parameters s [nq] in the frame of eqlb_facet_points;
    u_h = sum_j l_j(s_q) u[dof_j], ascending j, every product rounded on its own, l of facet_basis; u_ext None: 0."""
    s = np.asarray(s, dtype=np.float64).ravel()
    f = np.asarray(facets, dtype=np.int64).ravel()
    # the frame of eqlb_facet_points: the facet seen from its one cell, the low local vertex first; the facet's own
    # frame has 0 at the lower node id, so its parameter is s or 1 - s
    cells = mesh.facet_cells[mesh.facet_cells_offsets[f]]
    lf = np.argmax(mesh.cell_facets[cells] == f[:, None], axis=1)
    va, vb = np.where(lf == 0, 1, 0), np.where(lf == 2, 1, 2)
    rows = np.arange(f.size)
    same = mesh.cell_nodes[cells][rows, va] < mesh.cell_nodes[cells][rows, vb]
    B = np.where(same[:, None, None], facet_basis(p, s)[None], facet_basis(p, 1.0 - s)[None])   # [n, nq, p+1]
    uu = np.asarray(u, dtype=np.float64)[facet_dofs(mesh, p, f)]             # [n, p+1]
    v = B[:, :, 0] * uu[:, None, 0]
    for j in range(1, p + 1):
        v = v + B[:, :, j] * uu[:, None, j]
    if u_ext is not None:
        v = v - np.asarray(u_ext, dtype=np.float64).reshape(v.shape)
    return np.asarray(facet_alpha, dtype=np.float64).ravel()[:, None] * v


SPRING_ALLOWANCE = 2.0 ** -49   # of the semidefiniteness test of a spring tensor (the head of this file)


def spring_list(who, mesh, facets, k=1.0, facet_k=None):
    """(facets int64 [n], K [n, 3]) of set_springs in the order given, or (None, None) for an empty list; the scalar k
    stands for K = k I.  Refused by facet, in this order: one that is no boundary facet of the mesh, one listed twice,
    an entry of K that is not finite, k00 < 0, k11 < 0, k01 k01 > (k00 k11) (1 + 2^-49)."""
    f = np.asarray([] if facets is None else facets, dtype=np.int64).ravel()
    if facet_k is None:
        kk = float(k)
        if not (kk >= 0.0 and np.isfinite(kk)):
            raise ValueError(f"{who}: k = {kk} is negative, NaN or infinite")
        K = np.tile(np.array([kk, 0.0, kk]), (f.size, 1))
    else:
        K = np.array(facet_k, dtype=np.float64)
        if K.size != 3 * f.size:
            raise ValueError(f"{who}: facet_k [nlist][3] expected")
        K = K.reshape(f.size, 3)
    fco = mesh.facet_cells_offsets
    seen = set()
    for i, v in enumerate(f):
        v = int(v)
        if v < 0 or v >= mesh.nfacets or fco[v + 1] - fco[v] != 1:
            raise ValueError(f"{who}: facets[{i}] = {v} is no boundary facet of the mesh")
        if v in seen:
            raise ValueError(f"{who}: facets[{i}] = {v} is listed twice")
        seen.add(v)
        k00, k01, k11 = (float(x) for x in K[i])
        if not (np.isfinite(k00) and np.isfinite(k01) and np.isfinite(k11)):
            raise ValueError(f"{who}: facet_k[{i}] = ({k00}, {k01}, {k11}) is not finite")
        if k00 < 0.0:
            raise ValueError(f"{who}: facet_k[{i}]: k00 = {k00} is negative")
        if k11 < 0.0:
            raise ValueError(f"{who}: facet_k[{i}]: k11 = {k11} is negative")
        if not spring_semidefinite(K[i])[0]:
            raise ValueError(f"{who}: facet_k[{i}] = ({k00}, {k01}, {k11}) is not positive semidefinite")
    return (None, None) if f.size == 0 else (f, K)


def spring_semidefinite(K):
    """[n] bool: not k01 k01 > (k00 k11) (1 + 2^-49) - the last of the tests of spring_list, on finite tensors with
    k00, k11 >= 0."""
    K = np.asarray(K, dtype=np.float64).reshape(-1, 3)
    return ~(K[:, 1] * K[:, 1] > (K[:, 0] * K[:, 2]) * (1.0 + SPRING_ALLOWANCE))


def spring_definite(K):
    """[n] bool: k00 > 0 and k01 k01 < (k00 k11) (1 - 2^-49), the test for a positive definite tensor."""
    K = np.asarray(K, dtype=np.float64).reshape(-1, 3)
    return (K[:, 0] > 0.0) & (K[:, 1] * K[:, 1] < (K[:, 0] * K[:, 2]) * (1.0 - SPRING_ALLOWANCE))


def facet_normals(mesh, facets):
    """[n, 2]: the outward unit normal of each listed boundary facet: (dy, -dx) / |E| of facet_nodes with the |E| of
    facet_lengths, turned away from the vertex of the facet's cell that lies opposite."""
    f = np.asarray(facets, dtype=np.int64).ravel()
    fco = mesh.facet_cells_offsets
    for i, v in enumerate(f):
        if v < 0 or v >= mesh.nfacets or fco[v + 1] - fco[v] != 1:
            raise ValueError(f"facet_normals: facets[{i}] = {int(v)} is no boundary facet of the mesh")
    fn = mesh.facet_nodes[f]
    xa, xb = mesh.x[fn[:, 0], :2], mesh.x[fn[:, 1], :2]
    length = facet_lengths(mesh, f)
    n = np.stack([(xb[:, 1] - xa[:, 1]) / length, -(xb[:, 0] - xa[:, 0]) / length], axis=1)
    cells = mesh.facet_cells[fco[f]]
    lf = np.argmax(mesh.cell_facets[cells] == f[:, None], axis=1)
    xo = mesh.x[mesh.cell_nodes[cells, lf], :2]
    inward = np.sum(n * (xa - xo), axis=1) < 0.0
    return np.where(inward[:, None], -n, n)


def spring_tensor(mesh, facets, kn, kt=0.0):
    """facet_k [n, 3] of K = kn n x n + kt t x t with n the outward unit normal of each listed boundary facet
    (facet_normals) and t = (-n1, n0); kn, kt scalars or one value per facet.  Entry (a, b) is (kn n_a) n_b + (kt t_a)
    t_b, every operation rounded on its own; with kt = 0 the second term is left out, so that the tensor is the rank-one
    product kn n_a n_b that spring_list's allowance is made for."""
    return spring_tensor_of_normals(facet_normals(mesh, np.asarray(facets, dtype=np.int64).ravel()), kn, kt)


def spring_tensor_of_normals(n, kn, kt=0.0):
    """spring_tensor on given unit normals n [m, 2]."""
    n = np.asarray(n, dtype=np.float64).reshape(-1, 2)
    t = np.stack([-n[:, 1], n[:, 0]], axis=1)
    kn = np.broadcast_to(np.asarray(kn, dtype=np.float64), n.shape[:1])
    kt = np.broadcast_to(np.asarray(kt, dtype=np.float64), n.shape[:1])
    out = np.empty((n.shape[0], 3))
    for c, (a, b) in enumerate(((0, 0), (0, 1), (1, 1))):
        vn = (kn * n[:, a]) * n[:, b]
        out[:, c] = np.where(kt == 0.0, vn, vn + (kt * t[:, a]) * t[:, b])
    return out


def spring_load(mesh, p, facets, facet_k, u_ext, quadrature_degree=None):
    """b_extra [2 ndofs], blocked, = int_E phi_i (K u_ext)_r over the listed boundary facets, on the host: BY DEFINITION
    traction_load with the traction t = K u_ext, bit for bit that call - row r gets the flux condition g_r = -t_r =
    -(k_r0 u_ext,0 + k_r1 u_ext,1), and neumann_load returns -int_E g phi_i (the sign convention written in
    traction_load).  facet_k [n, 3]; u_ext a callable (x, y) -> (values of component 0, values of component 1)."""
    from types import SimpleNamespace
    f = np.asarray(facets, dtype=np.int64).ravel()
    K = np.asarray(facet_k, dtype=np.float64).reshape(f.size, 3)

    def row(kr0, kr1):
        def value(x, y):
            u0, u1 = u_ext(x, y)
            return -(kr0 * np.asarray(u0, dtype=np.float64) + kr1 * np.asarray(u1, dtype=np.float64))
        return value
    bcs = [[SimpleNamespace(facets=[int(v)], scalar=True, value=row(float(kk[r]), float(kk[r + 1])))
            for v, kk in zip(f, K)] for r in range(2)]
    return traction_load(mesh, p, bcs, quadrature_degree)


def spring_flux(mesh, p, facets, facet_k, u, s, u_ext=None):
    """The statement of eqlb_elasticity_spring_flux: out [2, n, nq], out[r][i][q] = K_i[r][0] d_0 + K_i[r][1] d_1 with
    d_s = u_h,s(x_q) - u_ext[s][i][q] on the listed facets at the facet parameters s [nq] in the frame of
    eqlb_facet_points.  u [2 ndofs] blocked; u_h,s is robin_flux with alpha = 1 on component s (facet_basis, ascending
    j); the contraction with K is two products and one addition.  u_ext [2, n, nq] or None (0).  Row r is what row r of
    a stress handle takes as its flux condition: -sigma_r . n = (K (u_h - u_ext))_r."""
    s = np.asarray(s, dtype=np.float64).ravel()
    f = np.asarray(facets, dtype=np.int64).ravel()
    K = np.asarray(facet_k, dtype=np.float64).reshape(f.size, 3)
    uu = np.asarray(u, dtype=np.float64).reshape(-1, 2)
    ue = None if u_ext is None else np.asarray(u_ext, dtype=np.float64).reshape(2, f.size, s.size)
    one = np.ones(f.size)
    d = [robin_flux(mesh, p, f, one, np.ascontiguousarray(uu[:, c]), s, None if ue is None else ue[c])
         for c in range(2)]
    return np.stack([K[:, r, None] * d[0] + K[:, r + 1, None] * d[1] for r in range(2)])


def value_dg(p, degree_dg, cell_dofs, u, coeff=None, op=None, return_abs=False):
    """The statement of eqlb_primal_value_dg: out [nrhs, ncells * nd_d] from u [nrhs, ndofs] (or [ndofs]), cell_dofs
    [ncells, nd_p]; coeff [ncells] or None (no multiplication); op [nd_d, nd_p] replaces the built-in table."""
    T = value_table(p, degree_dg) if op is None else np.asarray(op, dtype=np.float64).reshape(nd_of(degree_dg), nd_of(p))
    cd = np.asarray(cell_dofs, dtype=np.int64).reshape(-1, nd_of(p))
    uu = np.asarray(u, dtype=np.float64)
    uu = uu.reshape(1, -1) if uu.ndim < 2 else uu
    out, Ab = [], []
    for r in range(uu.shape[0]):
        v, A = _sum_products(T, uu[r][cd])
        if coeff is not None:
            k = np.asarray(coeff, dtype=np.float64).ravel()[:, None]
            v, A = k * v, np.abs(k) * A
        out.append(v.ravel())
        Ab.append(A.ravel())
    return (np.stack(out), np.stack(Ab)) if return_abs else np.stack(out)


def reaction_coefficient(who, ncells, c=0.0, cell_c=None):
    """c_T [ncells] of set_reaction, or None where the term is switched off (c == 0 without an array).  A coefficient
    that is negative, NaN or infinite is refused, the cell named."""
    if cell_c is None:
        c = float(c)
        if not (c >= 0.0 and np.isfinite(c)):
            raise ValueError(f"{who}: c = {c} is negative, NaN or infinite")
        return None if c == 0.0 else np.full(ncells, c)
    cc = np.array(cell_c, dtype=np.float64).ravel()
    if cc.size != ncells:
        raise ValueError(f"{who}: cell_c [ncells] expected")
    bad = np.nonzero(~((cc >= 0.0) & np.isfinite(cc)))[0]
    if bad.size:
        raise ValueError(f"{who}: cell_c[{int(bad[0])}] = {cc[bad[0]]} is negative, NaN or infinite")
    return cc


def shear_coefficient(who, ncells, mu=1.0, cell_mu=None):
    """mu_T [ncells] of set_shear, or None where the term is switched off (mu == 1 without an array).  A coefficient
    that is zero, negative, NaN or infinite is refused, the cell named."""
    if cell_mu is None:
        mu = float(mu)
        if not (mu > 0.0 and np.isfinite(mu)):
            raise ValueError(f"{who}: mu = {mu} is zero, negative, NaN or infinite")
        return None if mu == 1.0 else np.full(ncells, mu)
    mm = np.array(cell_mu, dtype=np.float64).ravel()
    if mm.size != ncells:
        raise ValueError(f"{who}: cell_mu [ncells] expected")
    bad = np.nonzero(~((mm > 0.0) & np.isfinite(mm)))[0]
    if bad.size:
        raise ValueError(f"{who}: cell_mu[{int(bad[0])}] = {mm[bad[0]]} is zero, negative, NaN or infinite")
    return mm


def diffusion_tensor(who, ncells, cell_D=None):
    """D_T [ncells, 3] = (d00, d01, d11) of set_diffusion, or None where the term is switched off.  A cell with a value
    that is not finite, or where d00 > 0 and d00 d11 - d01^2 > 0 do not both hold, is refused, the cell named."""
    if cell_D is None:
        return None
    dd = np.array(cell_D, dtype=np.float64)
    if dd.size != 3 * ncells:
        raise ValueError(f"{who}: cell_D [ncells][3] expected")
    dd = dd.reshape(ncells, 3)
    fin = np.isfinite(dd).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        spd = (dd[:, 0] > 0.0) & (dd[:, 0] * dd[:, 2] - dd[:, 1] * dd[:, 1] > 0.0)
    bad = np.nonzero(~(fin & spd))[0]
    if bad.size:
        i = int(bad[0])
        why = "not finite" if not fin[i] else "not positive definite"
        raise ValueError(f"{who}: cell_D[{i}] = ({dd[i, 0]}, {dd[i, 1]}, {dd[i, 2]}) is {why}")
    return dd


def diffusion_min_eigenvalue(cell_D, coeff=None):
    """lambda_min(kappa_T D_T) [ncells] of cell_D [ncells, 3] = (d00, d01, d11) and the cell-wise kappa (None: 1):
    kappa ((d00 + d11) / 2 - sqrt(((d00 - d11) / 2)^2 + d01^2)), formed as det D / lambda_max with the accurate
    determinant of eqlb.check_eqlb_conditions.det_sym2, so that a small eigenvalue keeps its digits."""
    from ..eqlb.check_eqlb_conditions import det_sym2
    dd = np.asarray(cell_D, dtype=np.float64).reshape(-1, 3)
    m, h = 0.5 * (dd[:, 0] + dd[:, 2]), 0.5 * (dd[:, 0] - dd[:, 2])
    lmax = m + np.sqrt(h * h + dd[:, 1] * dd[:, 1])
    lmin = det_sym2(dd[:, 0], dd[:, 1], dd[:, 2]) / lmax
    return lmin if coeff is None else np.asarray(coeff, dtype=np.float64).ravel() * lmin


def diffusion_oscillation_weight(cell_D, coeff=None):
    """The factor 1 / sqrt(lambda_min(kappa_T D_T)) [ncells] that weights the data oscillation h_T / pi || f - Pi f ||_T
    of a cell in the energy norm of -div(kappa D grad u): hand it to cpp.oscillation as `korn` (the cell-wise factor of
    the oscillation term), or multiply the unweighted term by it.  A host array operation, no kernel."""
    return 1.0 / np.sqrt(diffusion_min_eigenvalue(cell_D, coeff))


def flux_dg_tensor(mesh, p, degree_dg, cell_dofs, u, cell_D, PG, coeff=None):
    """The statement of eqlb_primal_flux_dg_tensor, bit for bit: out [nrhs, ncells * nd_d * 2], the DG_d^2 DOFs of
    -kappa_T D_T grad(u_h) from u [nrhs, ndofs] (or [ndofs]), cell_dofs [ncells, nd_p], cell_D [ncells, 3] = (d00, d01,
    d11), coeff [ncells] or None (kappa = 1) and the table PG [2, nd_d, nd_p] (cpp.get_primal_table, or the caller's op).
      gref[n][X] = the nd_p products PG[X][n][i] u[cell_dofs[c][i]], each rounded, sorted ascending and added from the
                   smallest up (the sum of eqlb_primal_flux_dg, which depends on the set of products only)
      gx = K00 gref[n][0] + K10 gref[n][1],  gy = K01 gref[n][0] + K11 gref[n][1]     (K = J^-1 as PoissonOperator forms it)
      out[c][n]  = ((-kappa) (d00 gx + d01 gy), (-kappa) (d01 gx + d11 gy))
    every product and every sum rounded on its own."""
    nd, ndp = nd_of(degree_dg), nd_of(p)
    T = np.asarray(PG, dtype=np.float64).reshape(2, nd, ndp)
    cd = np.asarray(cell_dofs, dtype=np.int64).reshape(-1, ndp)
    uu = np.asarray(u, dtype=np.float64)
    uu = uu.reshape(1, -1) if uu.ndim < 2 else uu
    dd = diffusion_tensor("flux_dg_tensor", mesh.ncells, cell_D)
    if dd is None:
        raise ValueError("flux_dg_tensor: cell_D [ncells][3] expected")
    x, cn = mesh.x, mesh.cell_nodes
    J00, J01 = x[cn[:, 1], 0] - x[cn[:, 0], 0], x[cn[:, 2], 0] - x[cn[:, 0], 0]
    J10, J11 = x[cn[:, 1], 1] - x[cn[:, 0], 1], x[cn[:, 2], 1] - x[cn[:, 0], 1]
    idet = 1.0 / (J00 * J11 - J01 * J10)
    K00, K01, K10, K11 = (J11 * idet)[:, None], (-J01 * idet)[:, None], (-J10 * idet)[:, None], (J00 * idet)[:, None]
    kap = np.ones(mesh.ncells) if coeff is None else np.asarray(coeff, dtype=np.float64).ravel()
    mk = (-kap)[:, None]
    d00, d01, d11 = dd[:, 0, None], dd[:, 1, None], dd[:, 2, None]
    out = []
    for r in range(uu.shape[0]):
        prod = np.sort(T[:, None, :, :] * uu[r][cd][None, :, None, :], axis=3)        # [X, c, n, i] ascending in i
        g = prod[..., 0]
        for i in range(1, ndp):
            g = g + prod[..., i]
        gx, gy = K00 * g[0] + K10 * g[1], K01 * g[0] + K11 * g[1]
        f0, f1 = mk * (d00 * gx + d01 * gy), mk * (d01 * gx + d11 * gy)
        out.append(np.stack([f0, f1], axis=2).ravel())
    return np.stack(out)


def cross_table(p):
    """The table [nd_p, nd_p] as doubles, each entry rounded once."""
    return np.array([[float(v) for v in row] for row in cross_table_exact(p)])


def stiffness_table(p):
    """The table [3, nd_p, nd_p] as doubles, each entry rounded once."""
    return np.array([[[float(v) for v in row] for row in m] for m in stiffness_table_exact(p)])


def load_table(p, d):
    """The table [nd_p, nd_d] as doubles, each entry rounded once."""
    return np.array([[float(v) for v in row] for row in load_table_exact(p, d)])


def dirichlet_mask(mesh, p, facets):
    """fixed [ndofs] bool: the vertex and facet DOFs of the listed facets."""
    f = np.asarray(facets, dtype=np.int64).ravel()
    for i, v in enumerate(f):
        if v < 0 or v >= mesh.nfacets:
            raise ValueError(f"dirichlet_mask: facets[{i}] = {int(v)} is no facet of the mesh")
    ndofs = lagrange_dofmap(mesh, p)[1]
    fixed = np.zeros(ndofs, dtype=bool)
    fixed[mesh.facet_nodes[f].ravel()] = True
    for j in range(p - 1):
        fixed[mesh.nnodes + f * (p - 1) + j] = True
    return fixed


def neumann_load(mesh, p, bcs, quadrature_degree=None):
    """b_extra [ndofs] of a problem with prescribed normal flux: for every `fluxbc` of `bcs` with a callable value,
    -int_E g phi_i over its boundary facets E, g the normal flux sigma . n (the callable itself with scalar=True, else
    the outward normal component of its vector), by Gauss quadrature (default degree 2 p + 4) on the host - O(sqrt N)
    facets - in the numbering of lagrange_dofmap.  The flux-BC DOF table of the equilibrator cannot supply this vector:
    it stops at moment k - 1, and the trace of P_p needs moment p."""
    from ..elmtlib.quadrature import make_quadrature_interval
    cd, ndofs = lagrange_dofmap(mesh, p)
    b = np.zeros(ndofs)
    s, wq = make_quadrature_interval(2 * p + 4 if quadrature_degree is None else int(quadrature_degree))
    z = np.zeros_like(s)
    ref = (np.stack([1 - s, s], 1), np.stack([z, s], 1), np.stack([s, z], 1))    # facet 0, 1, 2 (eqlb/bcs.py)
    phi = [Lagrange(p).tabulate(pts)[0] for pts in ref]                          # [nq, nd]
    ends = ((1, 2), (0, 2), (0, 1))
    for bc in bcs:
        if getattr(bc, "value", None) is None:
            continue
        for f in np.asarray(bc.facets, dtype=np.int64).ravel():
            if f < 0 or f >= mesh.nfacets or mesh.facet_cells_offsets[f + 1] - mesh.facet_cells_offsets[f] != 1:
                raise ValueError(f"neumann_load: facet {int(f)} is no boundary facet of the mesh")
            c = int(mesh.facet_cells[mesh.facet_cells_offsets[f]])
            lf = int(np.nonzero(mesh.cell_facets[c] == f)[0][0])
            xc = mesh.x[mesh.cell_nodes[c], :2]
            xa, xb, xo = xc[ends[lf][0]], xc[ends[lf][1]], xc[lf]
            tvec = xb - xa
            length = float(np.hypot(*tvec))
            n = np.array([tvec[1], -tvec[0]]) / length
            if np.dot(n, xa - xo) < 0.0:
                n = -n
            xq = xc[0][None, :] + ref[lf] @ np.stack([xc[1] - xc[0], xc[2] - xc[0]])
            val = np.asarray(bc.value(xq[:, 0], xq[:, 1]), dtype=np.float64)
            if getattr(bc, "scalar", False):
                g = np.broadcast_to(val, s.shape)
            else:
                g = np.broadcast_to(val[0], s.shape) * n[0] + np.broadcast_to(val[1], s.shape) * n[1]
            np.add.at(b, cd[c], -length * ((wq * g) @ phi[lf]))
    return b


def _sum_products(T, v):
    """(val, A) [ncells, n]: sum_j T[i][j] v[c][j] in ascending j, products rounded one by one, and sum |T| |v|."""
    val = T[None, :, 0] * v[:, None, 0]
    A = np.abs(T[None, :, 0]) * np.abs(v[:, None, 0])
    for j in range(1, T.shape[1]):
        val = val + T[None, :, j] * v[:, None, j]
        A = A + np.abs(T[None, :, j]) * np.abs(v[:, None, j])
    return val, A


def csr_apply(indptr, indices, values, x, return_abs=False):
    """The statement of eqlb_csr_apply: y [n] with y[row] the sum of values[k] x[indices[k]] over the positions k of the
    row in ascending order: the first product starts the sum, then s = s + v x, each rounded on its own.  An empty row
    gives 0.0.  return_abs: also the same sum on the absolute values."""
    ip = np.asarray(indptr, dtype=np.int64)
    ix = np.asarray(indices, dtype=np.int64)
    v = np.asarray(values, dtype=np.float64)
    xx = np.asarray(x, dtype=np.float64)
    n = ip.size - 1
    cnt = np.diff(ip)
    y, A = np.zeros(n), np.zeros(n)
    for k in range(int(cnt.max()) if n else 0):
        sel = np.nonzero(cnt > k)[0]
        pos = ip[sel] + k
        t = v[pos] * xx[ix[pos]]
        ta = np.abs(v[pos]) * np.abs(xx[ix[pos]])
        y[sel] = t if k == 0 else y[sel] + t
        A[sel] = ta if k == 0 else A[sel] + ta
    return (y, A) if return_abs else y


class PoissonOperator:
    """The statements on one mesh: PoissonOperator(mesh, p, coeff=None), coeff [ncells] the cell-wise kappa."""

    def __init__(self, mesh, p, coeff=None):
        if p < 1 or p > 4:
            raise ValueError(f"PoissonOperator: p = {p} outside 1 ... 4")
        self.mesh, self.p, self.nd = mesh, p, nd_of(p)
        cd, self.ndofs = lagrange_dofmap(mesh, p)
        self.cell_dofs = cd.astype(np.int64)
        x, cn = mesh.x, mesh.cell_nodes
        J00, J01 = x[cn[:, 1], 0] - x[cn[:, 0], 0], x[cn[:, 2], 0] - x[cn[:, 0], 0]
        J10, J11 = x[cn[:, 1], 1] - x[cn[:, 0], 1], x[cn[:, 2], 1] - x[cn[:, 0], 1]
        det = J00 * J11 - J01 * J10
        idet = 1.0 / det
        K00, K01, K10, K11 = J11 * idet, -J01 * idet, -J10 * idet, J00 * idet
        self.K = ((K00, K01), (K10, K11))     # K[X][d]
        self.cell_D = None                    # (d00, d01, d11) [ncells, 3]; None: no diffusion tensor
        self._metric()
        self.adet = np.abs(det)
        kappa = np.ones(mesh.ncells) if coeff is None else np.asarray(coeff, dtype=np.float64).ravel()
        if kappa.size != mesh.ncells:
            raise ValueError("PoissonOperator: coeff [ncells] expected")
        self.w = kappa * self.adet
        self.S = stiffness_table(p)
        self.Mass = mass_table(p)
        self.wm = None                        # c_T |det| [ncells]; None: no reaction term
        self.fixed = np.zeros(self.ndofs, dtype=bool)
        self._slots()

    # the Robin term (the head of this file): None without it; else the list sorted by facet id
    robin_f = robin_alpha = robin_w = robin_dofs = None
    _robin_order = None

    def set_robin(self, facets, alpha=1.0, facet_alpha=None):
        """The operator gains int alpha u v over the listed boundary facets: alpha_f = facet_alpha [nlist] where given,
        else the scalar alpha.  An empty list switches the term off; a repeated call replaces the list; a refused one
        leaves the operator as it was.  A hierarchy with coarse=True has to be built again afterwards."""
        if self._bs != 1:
            raise ValueError("set_robin: provided for PoissonOperator only")
        f, al = robin_list("set_robin", self.mesh, facets, alpha, facet_alpha)
        if f is None:
            self.robin_f = self.robin_alpha = self.robin_w = self.robin_dofs = self._robin_order = None
            return
        w = al * facet_lengths(self.mesh, f)
        order = np.argsort(f, kind="stable")
        self._robin_order = order
        self.robin_f, self.robin_alpha, self.robin_w = f[order], al[order], w[order]
        self.robin_dofs = facet_dofs(self.mesh, self.p, self.robin_f)

    def robin_weights(self):
        """w_f [nlist] in the order of the list given to set_robin (empty without the term)."""
        if self.robin_f is None:
            return np.zeros(0)
        out = np.empty(self.robin_w.size)
        out[self._robin_order] = self.robin_w
        return out

    def robin_positive(self):
        """Whether the term is on with some alpha_f > 0: the operator is then definite without a fixed DOF."""
        return self.robin_f is not None and bool((self.robin_alpha > 0.0).any())

    def _add_robin(self, y, u, A=None):
        """y (and A, the absolute sums) with the facet values t_f[i] added, facets ascending, one addition each."""
        if self.robin_f is None:
            return y, A
        FM = facet_mass_table(self.p)
        t, tA = _sum_products(FM, np.asarray(u, dtype=np.float64)[self.robin_dofs])
        t, tA = self.robin_w[:, None] * t, self.robin_w[:, None] * tA
        for k in range(self.robin_f.size):          # (a row lies in several facets: one after the other)
            d = self.robin_dofs[k]
            y[d] = y[d] + t[k]
            if A is not None:
                A[d] = A[d] + tA[k]
        return y, A

    def _slots(self):
        """slot lists of the owner sum: for every vertex and facet DOF the flat indices c * nd + i of its y_loc entries
        in the order of the node -> cell / facet -> cell table; the local index comes from matching ids."""
        m, p, nd = self.mesh, self.p, self.nd
        cd = self.cell_dofs
        nn, nf, ne = m.nnodes, m.nfacets, p - 1
        off, slots = [0], []
        for n in range(nn):
            for c in m.node_cells[m.node_cells_offsets[n]:m.node_cells_offsets[n + 1]]:
                slots.append(int(c) * nd + int(np.nonzero(cd[c] == n)[0][0]))
            off.append(len(slots))
        for f in range(nf):
            cells = m.facet_cells[m.facet_cells_offsets[f]:m.facet_cells_offsets[f + 1]]
            for j in range(ne):
                d = nn + f * ne + j
                for c in cells:
                    slots.append(int(c) * nd + int(np.nonzero(cd[c] == d)[0][0]))
                off.append(len(slots))
        self.slot_off = np.array(off, dtype=np.int64)
        self.slots = np.array(slots, dtype=np.int64)
        self.nshared = nn + nf * ne

    def set_dirichlet(self, facets):
        """A repeated call replaces the mask."""
        self.fixed = dirichlet_mask(self.mesh, self.p, facets)

    def set_reaction(self, c=0.0, cell_c=None):
        """The operator gains + c u: c_T = cell_c [ncells] where given, else the scalar c on every cell.  c == 0 without
        an array switches the term off; a repeated call replaces the coefficient."""
        cc = reaction_coefficient("set_reaction", self.mesh.ncells, c, cell_c)
        self.wm = None if cc is None else cc * self.adet

    def _metric(self):
        """C00, C01, C11 [ncells]: K K^T, or K D K^T with the tensor of set_diffusion (the head of this file).  Cabs: what
        return_abs puts in their place: |C| without the tensor, as before it existed; with it the same two-stage sum on
        the absolute values of K and D, since K D K^T can cancel where K K^T cannot."""
        K = self.K
        if self.cell_D is None:
            self.C00 = K[0][0] * K[0][0] + K[0][1] * K[0][1]
            self.C01 = K[0][0] * K[1][0] + K[0][1] * K[1][1]
            self.C11 = K[1][0] * K[1][0] + K[1][1] * K[1][1]
            self.Cabs = (np.abs(self.C00), np.abs(self.C01), np.abs(self.C11))
            return
        d00, d01, d11 = self.cell_D[:, 0], self.cell_D[:, 1], self.cell_D[:, 2]
        D = ((d00, d01), (d01, d11))
        T = [[K[X][0] * D[0][b] + K[X][1] * D[1][b] for b in range(2)] for X in range(2)]
        self.C00 = T[0][0] * K[0][0] + T[0][1] * K[0][1]
        self.C01 = T[0][0] * K[1][0] + T[0][1] * K[1][1]
        self.C11 = T[1][0] * K[1][0] + T[1][1] * K[1][1]
        Ka = [[np.abs(v) for v in row] for row in K]
        Da = [[np.abs(v) for v in row] for row in D]
        Ta = [[Ka[X][0] * Da[0][b] + Ka[X][1] * Da[1][b] for b in range(2)] for X in range(2)]
        self.Cabs = (Ta[0][0] * Ka[0][0] + Ta[0][1] * Ka[0][1], Ta[0][0] * Ka[1][0] + Ta[0][1] * Ka[1][1],
                     Ta[1][0] * Ka[1][0] + Ta[1][1] * Ka[1][1])

    def set_diffusion(self, cell_D=None):
        """The operator becomes -div(kappa D grad u): cell_D [ncells, 3] = (d00, d01, d11) of the symmetric positive
        definite tensor of each cell; None switches the term off.  A repeated call replaces the tensor; a refused one
        leaves the operator as it was.  A hierarchy with coarse=True has to be built again afterwards (on the device:
        Multilevel.set_coarse(True)).  D crosses a refinement through Refinement.prolong_dg(0, cell_D.ravel(), bs=3)."""
        self.cell_D = diffusion_tensor("set_diffusion", self.mesh.ncells, cell_D)
        self._metric()

    def _add_reaction(self, val, A, m, mA):
        """val + wm m on [ncells, nd] (A: the same with absolute values, or None); unchanged without the term."""
        if self.wm is None:
            return val, A
        wm = self.wm[:, None]
        return val + wm * m, (None if A is None else A + wm * mA)

    # ---- the statements ----
    def _combine(self, t, w, A=None):
        """w ((C00 t0 + C01 t1) + C11 t2) on [3][ncells, nd]; with A the same with absolute values."""
        c0, c1, c2 = self.C00[:, None], self.C01[:, None], self.C11[:, None]
        val = w[:, None] * ((c0 * t[0] + c1 * t[1]) + c2 * t[2])
        if A is None:
            return val
        a0, a1, a2 = (v[:, None] for v in self.Cabs)
        return val, np.abs(w)[:, None] * ((a0 * A[0] + a1 * A[1]) + a2 * A[2])

    def cell_product(self, u, return_abs=False):
        """y_loc [ncells, nd]."""
        uc = np.asarray(u, dtype=np.float64)[self.cell_dofs]
        t, A = zip(*[_sum_products(self.S[m], uc) for m in range(3)])
        val, Ab = self._combine(t, self.w, A)
        if self.wm is not None:
            val, Ab = self._add_reaction(val, Ab, *_sum_products(self.Mass, uc))
        return (val, Ab) if return_abs else val

    def owner_sum(self, y_loc, return_abs=False):
        """y [ndofs] from y_loc [ncells, nd]."""
        flat = np.ascontiguousarray(y_loc, dtype=np.float64).ravel()
        y = np.zeros(self.ndofs)
        A = np.zeros(self.ndofs)
        ni = self.nd - 3 * self.p
        y[self.nshared:] = np.asarray(y_loc)[:, 3 * self.p:].ravel() if ni else 0.0
        A[self.nshared:] = np.abs(y[self.nshared:])
        off = self.slot_off
        cnt = np.diff(off)
        first = self.slots[off[:-1]]
        y[:self.nshared] = flat[first]
        A[:self.nshared] = np.abs(flat[first])
        for k in range(1, int(cnt.max())):
            sel = np.nonzero(cnt > k)[0]
            v = flat[self.slots[off[sel] + k]]
            y[sel] = y[sel] + v
            A[sel] = A[sel] + np.abs(v)
        return (y, A) if return_abs else y

    def apply(self, u, masked=False, return_abs=False):
        """y = A u; masked: 0 on the fixed rows."""
        if return_abs:
            yl, Al = self.cell_product(u, True)
            y = self.owner_sum(yl)
            A = self.owner_sum(Al)
        else:
            y, A = self.owner_sum(self.cell_product(u)), None
        y, A = self._add_robin(y, u, A)
        if masked:
            y[self.fixed] = 0.0
        return (y, A) if return_abs else y

    def load(self, degree_dg, rhs_dg, b_extra=None, return_abs=False):
        """b [ndofs] from rhs_dg [ncells * nd_d] (DG_d nodal values)."""
        if degree_dg < 0 or degree_dg > 3:
            raise ValueError(f"load: degree_dg = {degree_dg} outside 0 ... 3")
        L = load_table(self.p, degree_dg)
        f = np.asarray(rhs_dg, dtype=np.float64).reshape(self.mesh.ncells, nd_of(degree_dg))
        s, A = _sum_products(L, f)
        b = self.owner_sum(self.adet[:, None] * s)
        Ab = self.owner_sum(self.adet[:, None] * A)
        if b_extra is not None:
            e = np.asarray(b_extra, dtype=np.float64)
            b = b + e
            Ab = Ab + np.abs(e)
        return (b, Ab) if return_abs else b

    def diagonal(self, return_abs=False):
        """The diagonal of the cell matrices through the owner sum."""
        t = [np.broadcast_to(np.diagonal(self.S[m])[None, :], (self.mesh.ncells, self.nd)) for m in range(3)]
        val, A = self._combine(t, self.w, [np.abs(x) for x in t])
        md = np.broadcast_to(np.diagonal(self.Mass)[None, :], (self.mesh.ncells, self.nd))
        val, A = self._add_reaction(val, A, md, md)
        d, dA = self.owner_sum(val), self.owner_sum(A)
        if self.robin_f is not None:
            fm = np.diagonal(facet_mass_table(self.p))
            for k in range(self.robin_f.size):
                rows = self.robin_dofs[k]
                d[rows] = d[rows] + self.robin_w[k] * fm
                dA[rows] = dA[rows] + self.robin_w[k] * fm
        return (d, dA) if return_abs else d

    # ---- the assembled matrix (the head of this file) ----
    _bs = 1

    def _pattern(self):
        """(skey, srow, scol, sptr): the scalar pattern - the sorted distinct pairs (d, d') of DOFs with a common cell as
        keys d ndofs + d', rows, columns and row offsets [ndofs + 1]."""
        if getattr(self, "_pat", None) is None:
            cd, nd, n = self.cell_dofs, self.nd, self.ndofs
            key = np.unique(np.repeat(cd, nd, axis=1).ravel() * n + np.tile(cd, (1, nd)).ravel())
            srow = key // n
            self._pat = (key, srow, key % n, np.searchsorted(srow, np.arange(n + 1)).astype(np.int64))
        return self._pat

    def _cell_entries(self):
        """(E, |E|) [ncells, nd, nd, 1, 1]: entry (i, j) of the cell matrices by the rule of `diagonal`."""
        nc, nn = self.mesh.ncells, self.nd * self.nd
        t = [np.broadcast_to(self.S[m].ravel()[None, :], (nc, nn)) for m in range(3)]
        val, A = self._combine(t, self.w, [np.abs(x) for x in t])
        if self.cell_D is None:
            # an entry is compared on its own: C01 = K00 K10 + K01 K11 can cancel, which |C01| (Cabs) does not show
            Ka = [[np.abs(v)[:, None] for v in row] for row in self.K]
            a0, a1, a2 = (Ka[0][0] * Ka[0][0] + Ka[0][1] * Ka[0][1], Ka[0][0] * Ka[1][0] + Ka[0][1] * Ka[1][1],
                          Ka[1][0] * Ka[1][0] + Ka[1][1] * Ka[1][1])
            A = np.abs(self.w)[:, None] * ((a0 * np.abs(t[0]) + a1 * np.abs(t[1])) + a2 * np.abs(t[2]))
        mm = np.broadcast_to(self.Mass.ravel()[None, :], (nc, nn))
        val, A = self._add_reaction(val, A, mm, np.abs(mm))
        shape = (nc, self.nd, self.nd, 1, 1)
        return val.reshape(shape), A.reshape(shape)

    def _add_facet_entries(self, V, VA, skey):
        """The facet term on top of the cell sums V [pairs, bs, bs] (VA: the absolute sums), facets ascending."""
        if self.robin_f is None:
            return
        FM = facet_mass_table(self.p)
        for k in range(self.robin_f.size):
            rows = self.robin_dofs[k]
            pos = np.searchsorted(skey, rows[:, None] * self.ndofs + rows[None, :])
            e = self.robin_w[k] * FM
            V[pos, 0, 0] = V[pos, 0, 0] + e
            VA[pos, 0, 0] = VA[pos, 0, 0] + e

    def matrix(self, eliminate=False, return_abs=False):
        """(indptr int64 [n + 1], indices int32 [nnz], values [nnz]), n = bs ndofs: the operator as CSR by the rule at the
        head of this file.  eliminate: P A P + (I - P) on the mask of set_dirichlet.  return_abs: a fourth array, the
        same sums on the absolute values of the terms."""
        bs, nd, n = self._bs, self.nd, self.ndofs
        skey, srow, scol, sptr = self._pattern()
        E, EA = self._cell_entries()
        V, VA = np.zeros((skey.size, bs, bs)), np.zeros((skey.size, bs, bs))
        seen = np.zeros(skey.size, dtype=bool)

        def add(d, c, i):
            pos = np.searchsorted(skey, d[:, None] * n + self.cell_dofs[c])                # [m, nd]
            old = seen[pos][:, :, None, None]
            V[pos] = np.where(old, V[pos] + E[c, i], E[c, i])
            VA[pos] = np.where(old, VA[pos] + EA[c, i], EA[c, i])
            seen[pos] = True

        off = self.slot_off
        cnt = np.diff(off)
        for k in range(int(cnt.max()) if cnt.size else 0):
            sel = np.nonzero(cnt > k)[0]
            flat = self.slots[off[sel] + k]
            add(sel, flat // nd, flat % nd)
        ni = nd - 3 * self.p
        if ni:
            q = np.arange(self.mesh.ncells * ni)
            add(self.nshared + q, q // ni, 3 * self.p + q % ni)
        self._add_facet_entries(V, VA, skey)
        # the blocked layout: row bs d + r holds the columns bs d' + s, s fastest
        length = np.diff(sptr)
        rows = np.arange(bs * n)
        indptr = np.concatenate([bs * bs * sptr[rows // bs] + (rows % bs) * bs * length[rows // bs], [bs * bs * skey.size]])
        k = np.arange(skey.size) - sptr[srow]
        r, s = np.arange(bs)[None, :, None], np.arange(bs)[None, None, :]
        pos = (bs * bs * sptr[srow] + bs * k)[:, None, None] + r * bs * length[srow][:, None, None] + s
        indices = np.zeros(bs * bs * skey.size, dtype=np.int32)
        values, vabs = np.zeros(indices.size), np.zeros(indices.size)
        indices[pos] = bs * scol[:, None, None] + s
        values[pos], vabs[pos] = V, VA
        if eliminate:
            row_of = np.repeat(rows, np.diff(indptr))
            fx = self.fixed[row_of] | self.fixed[indices]
            unit = np.where(row_of == indices, 1.0, 0.0)
            values, vabs = np.where(fx, unit, values), np.where(fx, unit, vabs)
        out = (indptr.astype(np.int64), indices, values)
        return out + (vabs,) if return_abs else out

    def residual(self, b, u, fixed=None, return_abs=False):
        """r = b - A u, 0 on the rows where `fixed` (default: the mask of set_dirichlet) is set."""
        fx = self.fixed if fixed is None else np.asarray(fixed, dtype=bool)
        bb = np.asarray(b, dtype=np.float64)
        if return_abs:
            y, A = self.apply(u, return_abs=True)
            A = A + np.abs(bb)
        else:
            y, A = self.apply(u), None
        r = bb - y
        r[fx] = 0.0
        if return_abs:
            A[fx] = 0.0
        return (r, A) if return_abs else r

    def reference_norm(self, b, u):
        """nb = || (b - A u^)_free ||_2 with u^ = u with its free rows set to 0: includes the lifting of the data."""
        uh = np.where(self.fixed, np.asarray(u, dtype=np.float64), 0.0)
        r = self.residual(b, uh)
        return float(np.sqrt(np.sum(r * r)))

    def pcg(self, b, u, rtol=1e-8, atol=0.0, maxit=1000):
        """Jacobi-preconditioned CG from the start u, whose fixed rows hold the Dirichlet values (untouched).
        tol = max(rtol nb, atol).  When the recurrence residual reaches tol the true residual b - A u is computed with
        one more product: above tol it replaces the recurrence residual and the iteration goes on.  Returns (u, info)
        with info = dict(iterations, converged, nb, rnorm, replacements, breakdown) as eqlb_primal_solve."""
        if maxit < 1:
            raise ValueError(f"pcg: maxit = {maxit}")
        if not (rtol >= 0.0 and atol >= 0.0):
            raise ValueError(f"pcg: rtol = {rtol}, atol = {atol} negative or NaN")
        if not self.fixed.any() and not self.robin_positive():
            raise ValueError("pcg: singular: no Dirichlet DOF")
        u = np.array(u, dtype=np.float64)
        b = np.asarray(b, dtype=np.float64)
        nb = self.reference_norm(b, u)
        tol = max(rtol * nb, atol)
        info = dict(iterations=0, converged=0, nb=nb, rnorm=nb, replacements=0, breakdown=0)
        if tol == 0.0 and nb == 0.0:
            u[~self.fixed] = 0.0
            info.update(converged=1, rnorm=0.0)
            return u, info
        diag = self.diagonal()
        r = self.residual(b, u)
        rr = np.sum(r * r)
        if np.sqrt(rr) <= tol:
            info.update(converged=1, rnorm=float(np.sqrt(rr)))
            return u, info
        z = r / diag
        rho = np.sum(r * z)
        d = z.copy()
        for it in range(1, maxit + 1):
            q = self.apply(d, masked=True)
            dq = np.sum(d * q)
            if not dq > 0.0:
                info["breakdown"] = 1
                break
            alpha = rho / dq
            u = u + alpha * d
            r = r - alpha * q
            info["iterations"] = it
            rr = np.sum(r * r)
            if np.sqrt(rr) <= tol:
                rt = self.residual(b, u)
                rr = np.sum(rt * rt)
                if np.sqrt(rr) <= tol:
                    info["converged"] = 1
                    break
                r = rt
                info["replacements"] += 1
            z = r / diag
            rho_new = np.sum(r * z)
            beta = rho_new / rho
            rho = rho_new
            d = z + beta * d
        rt = self.residual(b, u)
        info["rnorm"] = float(np.sqrt(np.sum(rt * rt)))
        return u, info

    def pcg_many(self, B, U, rtol=1e-8, atol=0.0, maxit=1000):
        """Several right-hand sides B [nrhs][ndofs] from the starts U [nrhs][ndofs]: BY DEFINITION the loop over the
        columns of pcg - eqlb_primal_solve_many has no statement of its own.  Returns (U, [info_c])."""
        return pcg_columns(self.pcg, B, U, rtol, atol, maxit)


def pcg_columns(pcg, B, U, rtol, atol, maxit):
    """(U, [info_c]) with (U[c], info_c) = pcg(B[c], U[c], ...): the statement of the *_many solves."""
    B = np.asarray(B, dtype=np.float64)
    U = np.asarray(U, dtype=np.float64)
    if B.ndim != 2 or B.shape[0] < 1 or U.shape != B.shape:
        raise ValueError(f"pcg_many: B {B.shape} and U {U.shape} are not two arrays [nrhs][ndofs], nrhs >= 1")
    out = [pcg(B[c], U[c], rtol=rtol, atol=atol, maxit=maxit) for c in range(B.shape[0])]
    return np.stack([u for u, _ in out]), [info for _, info in out]


def traction_load(mesh, p, bcs_rows, quadrature_degree=None):
    """b_extra [2 ndofs], blocked, of an elasticity problem with prescribed tractions: bcs_rows = (bcs_0, bcs_1), the
    lists of `fluxbc` objects of the two stress rows; b_extra[2 d + r] = neumann_load(mesh, p, bcs_r)[d].  Row r of a
    stress handle equilibrates -sigma_r, so its flux boundary condition prescribes -sigma_r . n = -t_r, and
    neumann_load returns -int_E g phi_i: with g = -t_r that is +int_E t_r phi_i, the traction term of the weak form - the
    sign is already the one neumann_load uses, and the same objects serve the equilibrator and this load."""
    if len(bcs_rows) != 2:
        raise ValueError("traction_load: two lists of boundary conditions expected, one per stress row")
    rows = [neumann_load(mesh, p, bcs, quadrature_degree) for bcs in bcs_rows]
    return np.ascontiguousarray(np.stack(rows, axis=1).ravel())


class ElasticityOperator(PoissonOperator):
    """The statements of -div(2 eps(u) + pi_1 div(u) I) = f on one mesh: ElasticityOperator(mesh, p, pi_1=1.0,
    cell_pi1=None), cell_pi1 [ncells] the cell-wise pi_1 (else the scalar).  Vectors are blocked, [2 ndofs]; `ndofs`
    is the scalar count.  owner_sum, residual, reference_norm and pcg are those of PoissonOperator on the blocked
    vectors."""

    def __init__(self, mesh, p, pi_1=1.0, cell_pi1=None):
        if p < 1 or p > 4:
            raise ValueError(f"ElasticityOperator: p = {p} outside 1 ... 4")
        self.mesh, self.p, self.nd = mesh, p, nd_of(p)
        cd, self.ndofs = lagrange_dofmap(mesh, p)
        self.cell_dofs = cd.astype(np.int64)
        x, cn = mesh.x, mesh.cell_nodes
        J00, J01 = x[cn[:, 1], 0] - x[cn[:, 0], 0], x[cn[:, 2], 0] - x[cn[:, 0], 0]
        J10, J11 = x[cn[:, 1], 1] - x[cn[:, 0], 1], x[cn[:, 2], 1] - x[cn[:, 0], 1]
        det = J00 * J11 - J01 * J10
        idet = 1.0 / det
        K = ((J11 * idet, -J01 * idet), (-J10 * idet, J00 * idet))             # K[X][d]
        self.Q = [[[K[X][a] * K[Y][b] for X in range(2) for Y in range(2)] for b in range(2)] for a in range(2)]
        self.adet = np.abs(det)
        if cell_pi1 is None:
            self.pi = np.full(mesh.ncells, float(pi_1))
        else:
            self.pi = np.asarray(cell_pi1, dtype=np.float64).ravel()
            if self.pi.size != mesh.ncells:
                raise ValueError("ElasticityOperator: cell_pi1 [ncells] expected")
        S = stiffness_table(p)
        C = cross_table(p)
        self.M = (S[0], C, np.ascontiguousarray(C.T), S[2])                     # M_00, M_01, M_10, M_11
        self.Mass = mass_table(p)
        self.wm = None
        self.mu = None                        # mu_T [ncells]; None: no shear modulus (mu = 1)
        self.fixed = np.zeros(2 * self.ndofs, dtype=bool)
        self._slots()

    def set_diffusion(self, cell_D=None):
        """The elasticity operator knows no diffusion tensor."""
        raise ValueError("set_diffusion: provided for PoissonOperator only")

    def set_shear(self, mu=1.0, cell_mu=None):
        """The stress becomes mu (2 eps(u) + pi_1 div(u) I): mu_T = cell_mu [ncells] where given, else the scalar mu on
        every cell, mu_T > 0.  mu == 1 without an array switches the term off; a repeated call replaces the coefficient.
        The reaction term of set_reaction is not scaled.  A DG_0 coefficient crosses a refinement through
        Refinement.prolong_dg(0, cell_mu)."""
        self.mu = shear_coefficient("set_shear", self.mesh.ncells, mu, cell_mu)

    def _scale_shear(self, val, A=None):
        """mu_T val on [ncells, nd] (A: the same, or None); unchanged without the term."""
        if self.mu is None:
            return val, A
        m = self.mu[:, None]
        return m * val, (None if A is None else m * A)

    # the spring term (the head of this file): None without it; else the list sorted by facet id
    spring_f = spring_k = spring_kw = spring_dofs = None
    _spring_order = None

    def set_springs(self, facets, k=1.0, facet_k=None):
        """The operator gains int_E v^T K u over the listed boundary facets: K_f = facet_k [nlist, 3] = (k00, k01, k11)
        where given, else k I.  An empty list switches the term off; a repeated call replaces the list; a refused one
        (spring_list) leaves the operator as it was.  A hierarchy with coarse=True has to be built again afterwards."""
        f, K = spring_list("set_springs", self.mesh, facets, k, facet_k)
        if f is None:
            self.spring_f = self.spring_k = self.spring_kw = self.spring_dofs = self._spring_order = None
            return
        kw = facet_lengths(self.mesh, f)[:, None] * K
        order = np.argsort(f, kind="stable")
        self._spring_order = order
        self.spring_f, self.spring_k, self.spring_kw = f[order], K[order], kw[order]
        self.spring_dofs = facet_dofs(self.mesh, self.p, self.spring_f)

    def spring_weights(self):
        """Kw_f [nlist, 3] in the order of the list given to set_springs (empty without the term)."""
        if self.spring_f is None:
            return np.zeros((0, 3))
        out = np.empty(self.spring_kw.shape)
        out[self._spring_order] = self.spring_kw
        return out

    def spring_positive(self):
        """Whether some listed facet has |E_f| > 0 and a positive definite K_f: the operator is then definite without a
        fixed DOF in either component."""
        if self.spring_f is None:
            return False
        return bool((spring_definite(self.spring_k) & (facet_lengths(self.mesh, self.spring_f) > 0.0)).any())

    robin_positive = spring_positive      # what pcg and Hierarchy ask a level before they call it singular

    def _spring_rows(self):
        """((Kw[0][0], Kw[0][1]), (Kw[1][0], Kw[1][1])), each [nlist, 1]."""
        kw = self.spring_kw
        return ((kw[:, 0:1], kw[:, 1:2]), (kw[:, 1:2], kw[:, 2:3]))

    def _add_robin(self, y, u, A=None):
        """y [2 ndofs] (and A, the absolute sums) with the facet values t_f[i][r] added, facets ascending, one addition
        each."""
        if self.spring_f is None:
            return y, A
        FM = facet_mass_table(self.p)
        uu = np.asarray(u, dtype=np.float64).reshape(self.ndofs, 2)[self.spring_dofs]      # [n, p+1, 2]
        m, mA = zip(*[_sum_products(FM, uu[:, :, s]) for s in range(2)])
        Kw = self._spring_rows()
        for r in range(2):
            t = Kw[r][0] * m[0] + Kw[r][1] * m[1]
            tA = np.abs(Kw[r][0]) * mA[0] + np.abs(Kw[r][1]) * mA[1]
            for k in range(self.spring_f.size):     # (a row lies in several facets: one after the other)
                e = 2 * self.spring_dofs[k] + r
                y[e] = y[e] + t[k]
                if A is not None:
                    A[e] = A[e] + tA[k]
        return y, A

    def _add_facet_entries(self, V, VA, skey):
        if self.spring_f is None:
            return
        FM = facet_mass_table(self.p)
        Kw = self._spring_rows()
        for k in range(self.spring_f.size):
            rows = self.spring_dofs[k]
            pos = np.searchsorted(skey, rows[:, None] * self.ndofs + rows[None, :])
            for r in range(2):
                for s in range(2):
                    e = Kw[r][s][k, 0] * FM
                    V[pos, r, s] = V[pos, r, s] + e
                    VA[pos, r, s] = VA[pos, r, s] + np.abs(e)

    def set_dirichlet(self, facets_row0, facets_row1):
        """Fixed are the rows 2 dof + r of the vertex and facet DOFs of the facets listed for component r (the facets
        with ft[r] == 1 of a stress handle's facet types).  A repeated call replaces the mask."""
        m = [dirichlet_mask(self.mesh, self.p, f) for f in (facets_row0, facets_row1)]
        self.fixed = np.ascontiguousarray(np.stack(m, axis=1).ravel())

    # ---- the statements ----
    def _D(self, g, a, b, A=None):
        """(Q0 g0 + Q1 g1) + (Q2 g2 + Q3 g3) on [ncells, nd]; with A the same with absolute values."""
        q = [v[:, None] for v in self.Q[a][b]]
        val = (q[0] * g[0] + q[1] * g[1]) + (q[2] * g[2] + q[3] * g[3])
        if A is None:
            return val
        q = [np.abs(v) for v in q]
        return val, (q[0] * A[0] + q[1] * A[1]) + (q[2] * A[2] + q[3] * A[3])

    def cell_product(self, u, return_abs=False):
        """y_loc [ncells, nd, 2]."""
        uc = np.asarray(u, dtype=np.float64).reshape(self.ndofs, 2)[self.cell_dofs]    # [c, j, s]
        D = [[[None, None], [None, None]] for _ in range(2)]                             # D[s][a][b] = (val, abs)
        for s in range(2):
            g, A = zip(*[_sum_products(self.M[m], uc[:, :, s]) for m in range(4)])
            for a in range(2):
                for b in range(2):
                    D[s][a][b] = self._D(g, a, b, A)
        w, pi = self.adet[:, None], self.pi[:, None]
        wa, pa = np.abs(w), np.abs(pi)
        v = lambda s, a, b: D[s][a][b][0]   # noqa: E731
        n = lambda s, a, b: D[s][a][b][1]   # noqa: E731
        y0 = w * (((v(0, 0, 0) + v(0, 1, 1)) + (v(0, 0, 0) + v(1, 1, 0))) + pi * (v(0, 0, 0) + v(1, 0, 1)))
        y1 = w * (((v(1, 0, 0) + v(1, 1, 1)) + (v(0, 0, 1) + v(1, 1, 1))) + pi * (v(0, 1, 0) + v(1, 1, 1)))
        ys = [self._scale_shear(y)[0] for y in (y0, y1)]
        mm = [_sum_products(self.Mass, uc[:, :, r]) for r in range(2)] if self.wm is not None else None
        if mm is not None:
            ys = [self._add_reaction(ys[r], None, *mm[r])[0] for r in range(2)]
        val = np.stack(ys, axis=2)
        if not return_abs:
            return val
        a0 = wa * (((n(0, 0, 0) + n(0, 1, 1)) + (n(0, 0, 0) + n(1, 1, 0))) + pa * (n(0, 0, 0) + n(1, 0, 1)))
        a1 = wa * (((n(1, 0, 0) + n(1, 1, 1)) + (n(0, 0, 1) + n(1, 1, 1))) + pa * (n(0, 1, 0) + n(1, 1, 1)))
        ab = [self._scale_shear(a0, a0)[1], self._scale_shear(a1, a1)[1]]
        if mm is not None:
            ab = [ab[r] + self.wm[:, None] * mm[r][1] for r in range(2)]
        return val, np.stack(ab, axis=2)

    def owner_sum(self, y_loc, return_abs=False):
        """y [2 ndofs] from y_loc [ncells, nd, 2]: the scalar owner sum per component."""
        yl = np.asarray(y_loc, dtype=np.float64)
        parts = [PoissonOperator.owner_sum(self, yl[:, :, r], True) for r in range(2)]
        y = np.ascontiguousarray(np.stack([q[0] for q in parts], axis=1).ravel())
        A = np.ascontiguousarray(np.stack([q[1] for q in parts], axis=1).ravel())
        return (y, A) if return_abs else y

    def load(self, degree_dg, rhs_dg, b_extra=None, return_abs=False):
        """b [2 ndofs] from rhs_dg [2][ncells * nd_d] (DG_d nodal values of the two components)."""
        if degree_dg < 0 or degree_dg > 3:
            raise ValueError(f"load: degree_dg = {degree_dg} outside 0 ... 3")
        L = load_table(self.p, degree_dg)
        f = np.asarray(rhs_dg, dtype=np.float64).reshape(2, self.mesh.ncells, nd_of(degree_dg))
        s, A = zip(*[_sum_products(L, f[r]) for r in range(2)])
        b = self.owner_sum(self.adet[:, None, None] * np.stack(s, axis=2))
        Ab = self.owner_sum(self.adet[:, None, None] * np.stack(A, axis=2))
        if b_extra is not None:
            e = np.asarray(b_extra, dtype=np.float64)
            b = b + e
            Ab = Ab + np.abs(e)
        return (b, Ab) if return_abs else b

    def diagonal(self, return_abs=False):
        """The diagonal of the cell matrices through the owner sum."""
        g = [np.broadcast_to(np.diagonal(self.M[m])[None, :], (self.mesh.ncells, self.nd)) for m in range(4)]
        ga = [np.abs(x) for x in g]
        D = [[self._D(g, a, b, ga) for b in range(2)] for a in range(2)]
        w, pi = self.adet[:, None], self.pi[:, None]
        val = [w * (((D[0][0][0] + D[1][1][0]) + D[r][r][0]) + pi * D[r][r][0]) for r in range(2)]
        A = [np.abs(w) * (((D[0][0][1] + D[1][1][1]) + D[r][r][1]) + np.abs(pi) * D[r][r][1]) for r in range(2)]
        md = np.broadcast_to(np.diagonal(self.Mass)[None, :], (self.mesh.ncells, self.nd))
        val, A = zip(*[self._scale_shear(val[r], A[r]) for r in range(2)])
        val, A = zip(*[self._add_reaction(val[r], A[r], md, md) for r in range(2)])
        d, dA = self.owner_sum(np.stack(val, axis=2)), self.owner_sum(np.stack(A, axis=2))
        if self.spring_f is not None:
            fm = np.diagonal(facet_mass_table(self.p))
            for k in range(self.spring_f.size):
                for r in range(2):
                    e = 2 * self.spring_dofs[k] + r
                    t = self.spring_kw[k, 2 * r] * fm
                    d[e] = d[e] + t
                    dA[e] = dA[e] + np.abs(t)
        return (d, dA) if return_abs else d

    _bs = 2

    def _cell_entries(self):
        """(E, |E|) [ncells, nd, nd, 2, 2]: entry ((i, r), (j, s)) of the cell matrices (the head of this file)."""
        nc, nn = self.mesh.ncells, self.nd * self.nd
        g = [np.broadcast_to(self.M[m].ravel()[None, :], (nc, nn)) for m in range(4)]      # M_10[i][j] = Cross[j][i]
        ga = [np.abs(x) for x in g]
        D = [[self._D(g, a, b, ga) for b in range(2)] for a in range(2)]
        w, pi = self.adet[:, None], self.pi[:, None]
        wa, pa = np.abs(w), np.abs(pi)
        mm = np.broadcast_to(self.Mass.ravel()[None, :], (nc, nn))
        E, EA = np.zeros((nc, nn, 2, 2)), np.zeros((nc, nn, 2, 2))
        for r in range(2):
            for s in range(2):
                if r == s:
                    val = w * (((D[0][0][0] + D[1][1][0]) + D[r][r][0]) + pi * D[r][r][0])
                    A = wa * (((D[0][0][1] + D[1][1][1]) + D[r][r][1]) + pa * D[r][r][1])
                else:
                    val = w * (D[s][r][0] + pi * D[r][s][0])
                    A = wa * (D[s][r][1] + pa * D[r][s][1])
                val, A = self._scale_shear(val, A)
                if r == s:
                    val, A = self._add_reaction(val, A, mm, np.abs(mm))
                E[:, :, r, s], EA[:, :, r, s] = val, A
        shape = (nc, self.nd, self.nd, 2, 2)
        return E.reshape(shape), EA.reshape(shape)

    def pcg(self, b, u, rtol=1e-8, atol=0.0, maxit=1000):
        """The CG of PoissonOperator.pcg on the blocked vectors (eqlb_elasticity_solve).  Each component needs a
        Dirichlet DOF, unless a spring facet with a positive definite tensor holds every rigid motion (spring_positive);
        a rotation the mask leaves free is the caller's responsibility."""
        for r in range(2):
            if not self.fixed[r::2].any() and not self.spring_positive():
                raise ValueError(f"pcg: singular: component {r} has no Dirichlet DOF")
        return PoissonOperator.pcg(self, b, u, rtol, atol, maxit)
