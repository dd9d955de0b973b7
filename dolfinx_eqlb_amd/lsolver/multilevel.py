"""The multilevel preconditioner of the P_p solves over a hierarchy of refined meshes - the statement of the rule.

The Jacobi-preconditioned CG of lsolver/primal.py needs O(1/h) iterations.  With the levels an adaptive loop leaves
behind (DeviceMesh.refine(..., keep_plan=True)), the additive multilevel diagonal scaling (BPX)

    z = sum_l  P_L ... P_{l+1}  D_l^-1  P_{l+1}^T ... P_L^T  r

brings that down to a count that hardly grows with the level: P_{l+1} the prolongation from level l to level l + 1
(mesh.transfer.prolong_lagrange), D_l the diagonal of the operator of level l.  It is symmetric positive definite on the
free rows by construction, has no damping parameter and needs no operator product.  This file defines, in numpy, what
the device path (eqlb_hierarchy_* of include/eqlb.h, csrc/eqlb_multilevel.hip) computes; restrict and precondition are
reproduced bit for bit, because nothing in them reduces across threads except owner sums.

  levels     ops[0] ... ops[L]: PoissonOperator or ElasticityOperator of lsolver/primal.py, coarsest first, with their
             masks (set_dirichlet); links[l] = (parent_cell, node_parent_facet) of the refinement ops[l].mesh ->
             ops[l + 1].mesh (or any object with these two attributes, such as cpp.Refinement)
  restrict   mesh.transfer.restrict_lagrange with the owner sum of the coarse operator, masked at the coarse level
  down       r_L = r with the fixed rows set to 0;  r_l = restrict(r_{l+1})
  coarsest   z_0 = r_0 / diag_0 on the free rows, 0 elsewhere
  up         z_{l+1} = prolong(z_l) + r_{l+1} / diag_{l+1} on the free rows of level l + 1, 0 on its fixed rows: the
             quotient and the sum are rounded singly
  pcg        PoissonOperator.pcg with z = precondition(r) in the place of z = r / diag: the same start, the same
             reference norm, the true residual decides, replacement.  One more breakdown: r . z <= 0 (or NaN)

One level is plain Jacobi.

Local smoothing (Hierarchy(ops, links, local=True); eqlb_hierarchy_set_local).  The sum above smooths every row of every
level.  Where an adaptive loop refines a few percent of the cells per step, most rows of level l + 1 carry the basis
function they carried on level l, and the full sum counts that function once per level it survives.  With local=True a
level l >= 1 smooths only the rows whose basis function is new or changed there:

  changed    a cell of level l whose parent has more than one child: np.bincount(parent_cell)[parent_cell] > 1 on
             links[l - 1]
  active     a scalar DOF of level l that belongs to a changed cell (mesh.transfer.lagrange_dofmap); row bs dof + r with
             its DOF; on level 0 every row
  down, coarsest   as above
  up         a fixed row is 0; an active free row is prolong(z_l)[row] + r_{l+1}[row] / diag_{l+1}[row], quotient and sum
             rounded singly; an inactive free row takes prolong(z_l)[row] as it is - no addition, a -0.0 stays -0.0

A cell with one child is its parent, so an inactive row is a unit row of the prolongation: its function is the one of
the level below.  The preconditioner is still a sum of P M P^T terms with M diagonal and non-negative and level 0 in
full, so it is symmetric; and it is positive definite on the free rows because every free fine row is reached: a DOF
that is new on a level lies in a bisected cell and is active there, and one that was there from the start is active on
level 0.  On uniformly refined levels every row is active and the result is that of local=False bit for bit.

Exact coarse-level solve (Hierarchy(ops, links, coarse=True); eqlb_hierarchy_set_coarse).  Level 0 is treated by its
diagonal alone above.  With coarse=True it is solved on its free rows by a dense factor, formed once:

  rows       the free rows of level 0 (~ops[0].fixed), ascending in the row index bs dof + r; their count is n
  matrix     column j of A_0 is ops[0].apply(e_rows[j], masked=True) restricted to rows; only the lower triangle is read
  factor     right-looking LDL^T without a square root; for k = 0 ... n - 1: d_k = a_kk; c_i = a_ik and l_i = c_i / d_k
             for i > k; a_ij <- a_ij - l_i c_j for i >= j > k; W starts as the identity and w_ij <- w_ij - l_i w_kj
             for i > k >= j.  Every product and every difference is rounded singly, so each entry sees k ascending.
             The result: d [n] and the unit lower triangular W = L^-1 [n][n]
  coarsest   z_0[rows] = W^T ((W r_0[rows]) / d), 0 on the fixed rows, in the place of z_0 = r_0 / diag_0:
             y_i = sum_{k <= i} w_ik r_k with k ascending, y_i / d_i, z_j = sum_{i >= j} w_ij y_i with i ascending; every
             sum starts from 0.0, products and sums are rounded singly
  down, up, local   as above

The preconditioner is the sum of P M_l P^T with M_0 = W^T D^-1 W, symmetric positive definite for any nonsingular W and
positive d whatever the rounding did; a pivot that is not > 0 is refused.  One level with coarse=True is the direct
solve as a preconditioner.  The factor is a snapshot of the mask and the coefficient of level 0 when it is first asked
for (coarse_factor, precondition).
"""

import numpy as np

from ..mesh.transfer import lagrange_dofmap, prolong_lagrange, restrict_lagrange
from .primal import PoissonOperator, pcg_columns


class Hierarchy:
    """Hierarchy(ops, links, local=False, coarse=False): the statements on a hierarchy of levels, coarsest first.
    local: smooth on the levels l >= 1 only the rows whose basis function is new or changed there; coarse: solve level 0
    exactly on its free rows by a dense LDL^T factor in the place of its diagonal (the head of this file)."""

    def __init__(self, ops, links, local=False, coarse=False):
        ops, links = list(ops), list(links)
        if len(ops) < 1 or len(links) != len(ops) - 1:
            raise ValueError("Hierarchy: one link per pair of neighbouring levels expected")
        if any(o.p != ops[0].p for o in ops):
            raise ValueError("Hierarchy: levels of different p")
        self.ops, self.p = ops, ops[0].p
        self.bs = ops[0].fixed.size // ops[0].ndofs
        self.links = [(lk.parent_cell, lk.node_parent_facet) if hasattr(lk, "parent_cell") else tuple(lk)
                      for lk in links]
        self.links = [(np.asarray(pc), np.asarray(npf)) for pc, npf in self.links]
        for l, (pc, _) in enumerate(self.links):
            if pc.size != ops[l + 1].mesh.ncells:
                raise ValueError(f"Hierarchy: link {l} does not fit the mesh of level {l + 1}")
        self._diag = [None] * len(ops)
        self.local = bool(local)
        self._active = [None] * len(ops)
        self.coarse = bool(coarse)
        self._factor = None
        if self.coarse:
            for c in range(self.bs):
                if not ops[0].fixed[c::self.bs].any() and not ops[0].robin_positive():
                    raise ValueError(f"Hierarchy: coarse=True: component {c} of level 0 has no Dirichlet DOF")

    @property
    def nlevels(self):
        return len(self.ops)

    def diag(self, level):
        if self._diag[level] is None:
            self._diag[level] = self.ops[level].diagonal()
        return self._diag[level]

    def active(self, level):
        """bool [bs * ndofs_level]: the rows the local rule smooths on `level` (local=True only)."""
        if not self.local:
            raise ValueError("Hierarchy.active: the hierarchy smooths every row (local=False)")
        if level < 0 or level >= self.nlevels:
            raise ValueError(f"Hierarchy.active: level = {level} outside 0 ... {self.nlevels - 1}")
        if self._active[level] is None:
            op = self.ops[level]
            if level == 0:
                dofs = np.ones(op.ndofs, dtype=bool)
            else:
                pc = self.links[level - 1][0].astype(np.int64)
                changed = np.bincount(pc)[pc] > 1
                cell_dofs, ndofs = lagrange_dofmap(op.mesh, self.p)
                dofs = np.zeros(ndofs, dtype=bool)
                dofs[cell_dofs[changed].ravel()] = True
            self._active[level] = np.repeat(dofs, self.bs)
        return self._active[level]

    def coarse_matrix(self):
        """(rows int32 [n], A_0 [n][n]): the free rows of level 0 and the operator of level 0 on them, column by column
        from apply (coarse=True or not)."""
        op = self.ops[0]
        rows = np.nonzero(~op.fixed)[0].astype(np.int32)
        A = np.zeros((rows.size, rows.size))
        e = np.zeros(op.fixed.size)
        for j, row in enumerate(rows):
            e[row] = 1.0
            A[:, j] = op.apply(e, masked=True)[rows]
            e[row] = 0.0
        return rows, A

    def coarse_factor(self):
        """(rows int32 [n], d [n], W [n][n]): the factor of the exact solve on level 0 (coarse=True only); W is unit
        lower triangular with zeros above the diagonal."""
        if not self.coarse:
            raise ValueError("Hierarchy.coarse_factor: level 0 is treated by its diagonal (coarse=False)")
        if self._factor is None:
            rows, A = self.coarse_matrix()
            n = rows.size
            A = np.tril(A)
            W, d = np.eye(n), np.zeros(n)
            for k in range(n):
                d[k] = A[k, k]
                if not d[k] > 0.0:
                    raise ValueError(f"Hierarchy.coarse_factor: singular: pivot {k} (row {rows[k]} of level 0) is "
                                     f"{d[k]}, not positive")
                c = A[k + 1:, k].copy()
                l = c / d[k]
                # (in chunks of rows, each up to its last column of the lower triangle: what lies above the diagonal
                # inside a chunk is computed too and never read)
                for i0 in range(k + 1, n, 256):
                    i1 = min(i0 + 256, n)
                    A[i0:i1, k + 1:i1] = A[i0:i1, k + 1:i1] - l[i0 - k - 1:i1 - k - 1, None] * c[None, :i1 - k - 1]
                W[k + 1:, :k + 1] = W[k + 1:, :k + 1] - l[:, None] * W[k, :k + 1][None, :]
            self._factor = (rows, d, W)
        return self._factor

    def coarse_solve(self, r0):
        """z_0 of the exact rule from r_0 [bs ndofs_0]."""
        rows, d, W = self.coarse_factor()
        n = rows.size
        r = np.asarray(r0, dtype=np.float64)[rows]
        y = np.zeros(n)
        for k in range(n):
            y[k:] = y[k:] + W[k:, k] * r[k]
        y = y / d
        z = np.zeros(n)
        for i in range(n):
            z[:i + 1] = z[:i + 1] + W[i, :i + 1] * y[i]
        z0 = np.zeros(self.ops[0].fixed.size)
        z0[rows] = z
        return z0

    def restrict(self, level, r_fine, masked=True, return_abs=False):
        """level + 1 -> level."""
        if level < 0 or level >= self.nlevels - 1:
            raise ValueError(f"Hierarchy.restrict: level = {level} outside 0 ... {self.nlevels - 2}")
        lo, hi = self.ops[level], self.ops[level + 1]
        pc, npf = self.links[level]
        return restrict_lagrange(lo.mesh, hi.mesh, pc, npf, self.p, r_fine, bs=self.bs,
                                 fixed=lo.fixed if masked else None, return_abs=return_abs, op=lo)

    def prolong(self, level, z):
        """level -> level + 1."""
        lo, hi = self.ops[level], self.ops[level + 1]
        pc, npf = self.links[level]
        return prolong_lagrange(lo.mesh, hi.mesh, pc, npf, self.p, z, bs=self.bs)

    def precondition(self, r):
        L = self.nlevels - 1
        rs = [None] * (L + 1)
        rs[L] = np.where(self.ops[L].fixed, 0.0, np.asarray(r, dtype=np.float64))
        for l in range(L - 1, -1, -1):
            rs[l] = self.restrict(l, rs[l + 1])
        if self.coarse:
            z = self.coarse_solve(rs[0])
        else:
            z = np.where(self.ops[0].fixed, 0.0, rs[0] / self.diag(0))
        for l in range(1, L + 1):
            t = self.prolong(l - 1, z)
            z = t + rs[l] / self.diag(l)
            if self.local:
                z = np.where(self.active(l), z, t)
            z = np.where(self.ops[l].fixed, 0.0, z)
        return z

    def pcg(self, b, u, rtol=1e-8, atol=0.0, maxit=1000):
        """The CG of PoissonOperator.pcg on the finest level with this preconditioner.  Returns (u, info) with the
        same keys."""
        op = self.ops[-1]
        if maxit < 1:
            raise ValueError(f"pcg: maxit = {maxit}")
        if not (rtol >= 0.0 and atol >= 0.0):
            raise ValueError(f"pcg: rtol = {rtol}, atol = {atol} negative or NaN")
        for c in range(self.bs):
            if not op.fixed[c::self.bs].any() and not op.robin_positive():
                raise ValueError("pcg: singular: no Dirichlet DOF")
        u = np.array(u, dtype=np.float64)
        b = np.asarray(b, dtype=np.float64)
        nb = PoissonOperator.reference_norm(op, b, u)
        tol = max(rtol * nb, atol)
        info = dict(iterations=0, converged=0, nb=nb, rnorm=nb, replacements=0, breakdown=0)
        if tol == 0.0 and nb == 0.0:
            u[~op.fixed] = 0.0
            info.update(converged=1, rnorm=0.0)
            return u, info
        r = op.residual(b, u)
        rr = np.sum(r * r)
        if np.sqrt(rr) <= tol:
            info.update(converged=1, rnorm=float(np.sqrt(rr)))
            return u, info
        z = self.precondition(r)
        rho = np.sum(r * z)
        if not rho > 0.0:
            info["breakdown"] = 1
            maxit = 0
        d = z.copy()
        for it in range(1, maxit + 1):
            q = op.apply(d, masked=True)
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
                rt = op.residual(b, u)
                rr = np.sum(rt * rt)
                if np.sqrt(rr) <= tol:
                    info["converged"] = 1
                    break
                r = rt
                info["replacements"] += 1
            z = self.precondition(r)
            rho_new = np.sum(r * z)
            if not rho_new > 0.0:
                info["breakdown"] = 1
                break
            beta = rho_new / rho
            rho = rho_new
            d = z + beta * d
        rt = op.residual(b, u)
        info["rnorm"] = float(np.sqrt(np.sum(rt * rt)))
        return u, info

    def pcg_many(self, B, U, rtol=1e-8, atol=0.0, maxit=1000):
        """Several right-hand sides B [nrhs][n] from the starts U [nrhs][n]: by definition the loop over the columns
        of pcg (eqlb_hierarchy_solve_many; scalar hierarchies only).  Returns (U, [info_c])."""
        if self.bs != 1:
            raise ValueError("pcg_many: several right-hand sides are provided for the Poisson operator only")
        return pcg_columns(self.pcg, B, U, rtol, atol, maxit)
