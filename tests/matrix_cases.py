"""Shared by tests/test_primal_matrix_host.py and tests/test_gpu_primal_matrix.py: the operators whose CSR matrix
(lsolver.primal: PoissonOperator.matrix, ElasticityOperator.matrix, csr_apply) is checked, term by term, the
independently rounded assembly each is compared with, and the counts of roundings that bound the comparisons.  No test
lives here.

The terms of a case (VARIANTS):
  poisson     none (kappa = 1) | kappa cell-wise | diff: kappa and the tensor D of diffusion_cases | react: c cell-wise |
              all: kappa, D and c
  elasticity  none (the scalar pi_1 = 3.5) | pi1 cell-wise | shear: pi_1 and mu cell-wise (three values) | react |
              all: pi_1, mu and c

entry_terms (the comparison of one ENTRY with the quadrature assembly), counted the way primal_cases.chain_terms and
elasticity_cases.chain_terms count one entry of A u, with what an entry does not have taken out:
  statement   the geometry (12; elasticity 20), the combination (5; elasticity D_ab 3 and the sums 5), the sum over the
              cells of the pair (at most `valence`, the diagonal of the hub) - no contraction with u: chain_terms - nd_p
  assembled   tabulation 2 (p + 3), geometry 12, quadrature nq + 4, (elasticity: the three terms 3,) the cells `valence` -
              no product with u: chain_terms - nd_p valence (elasticity 2 nd_p valence); and the step that the product
              with u used to cover: elmtlib.polynomials.evaluate forms each of the two tabulated factors of a quadrature
              product as a sum of up to nd_p monomials, c x^a y^b added one by one: + 2 nd_p.
  abs-sums    of ONE entry, each computation's own: the statement's from matrix(return_abs=True); the assembly's from
              assembled_abs() below, NOT the |A| of the case modules.  That |A| is formed from |g| with
              g = K dphi already summed, and dphi from its monomials already summed.  Both sums cancel (the coefficients
              of P_4 reach 128 / 3; K of aspect1000 spans six orders of magnitude), and a single entry is small enough
              for it to show: on the one cell of `triangle` at P_4 the assembly misses the exact integral 16 / 189 of
              entry (0, 9) by 35 * 2^-53 with |A| = 0.38, 91 roundings' worth; aspect1000 at P_2 reaches 3.0 times
              the bound taken with |A|.  assembled_abs() takes the absolute values before those sums, as the rule asks
              ("the same sum with the absolute values of the terms"), and is >= |A| entry by entry.
  terms       diffusion + 3, + 3 (diffusion_cases.chain_terms); reaction + 1, + 1 (reaction_cases.chain_terms); shear + 1
              for the statement and + the number of distinct values for the assembly (tests/test_primal_shear_host.py)

chain (the comparison of csr_apply(matrix, x) with the matrix-free apply(x), both bounded by the ONE abs-sum of
apply(x, return_abs=True)): the roundings along the longest chain of the two computations, added, since either may err
by its own count times 2^-53 of (to first order) the same sum of absolute values:
  matrix-free the chain of chain_terms: geometry, contraction nd_p, combination, owner sum `valence`, + the terms
  assembled   per entry: geometry, combination, + the terms; per cell sum: `valence`; per row: the product with x 1 and
              the sum over the row `rowlen`
"""

import numpy as np

import diffusion_cases as dc
import elasticity_cases as ec
import primal_cases as pc
import primal_mesh_cases as pm
import reaction_cases as rc
import shear_cases as sc

U = pc.U
VARIANTS = {"poisson": ("none", "kappa", "diff", "react", "all"), "elasticity": ("none", "pi1", "shear", "react", "all")}
HOST_MESHES = ("triangle", "right1", "bowtie", "two_parts", "hole", "disk100", "delaunay", "aspect1000", "tiny_far", "huge")
PI_SCALAR = 3.5
# one pass of the grid-stride kernels of csrc/eqlb_primal_matrix.hip: pairs (fill, export, rows) and rows (csr_apply)
PAIRS_PER_PASS = 2048 * 256
ROWS_PER_PASS = 512 * 256


def mu_of(ncells, seed=41):
    """cell-wise mu with three distinct values (the assembly of shear_cases.assemble_mu runs once per value)"""
    return np.array([0.25, 1.0, 40.0])[np.random.default_rng(seed).integers(0, 3, ncells)]


def coefficients(problem, mesh, variant):
    """dict of the cell-wise data of a case: kappa / pi1 (None: 1 / the scalar), D, mu, c (None: term off)"""
    n = mesh.ncells
    k = dict(coeff=None, D=None, mu=None, c=None)
    if problem == "poisson":
        if variant in ("kappa", "diff", "all"):
            k["coeff"] = pc.kappa_of(n)
        if variant in ("diff", "all"):
            k["D"] = dc.tensor_of("random", mesh, 1e-2)
    else:
        if variant in ("pi1", "shear", "all"):
            k["coeff"] = ec.pi1_of(n)
        if variant in ("shear", "all"):
            k["mu"] = mu_of(n)
    if variant in ("react", "all"):
        k["c"] = rc.c_of(n)
    return k


def statement(problem, mesh, p, variant, layout="all"):
    """(the numpy statement with its terms and mask, the coefficients, the arguments of set_dirichlet)"""
    from dolfinx_eqlb_amd.lsolver import primal
    k = coefficients(problem, mesh, variant)
    if problem == "poisson":
        op = primal.PoissonOperator(mesh, p, k["coeff"])
        if k["D"] is not None:
            op.set_diffusion(k["D"])
        args = (pm.dirichlet_facets(mesh, layout),)
    else:
        op = primal.ElasticityOperator(mesh, p, PI_SCALAR, k["coeff"])
        if k["mu"] is not None:
            op.set_shear(cell_mu=k["mu"])
        args = tuple(pm.elasticity_lists(mesh, layout))
    if k["c"] is not None:
        op.set_reaction(cell_c=k["c"])
    op.set_dirichlet(*args)
    return op, k, args


def device_handle(cpp, dm, problem, p, k, args):
    """the device handle with the terms and the mask of statement()"""
    if problem == "poisson":
        h = cpp.PrimalPoisson(dm, p, k["coeff"])
        if k["D"] is not None:
            h.set_diffusion(k["D"])
    else:
        h = cpp.PrimalElasticity(dm, p, PI_SCALAR, k["coeff"])
        if k["mu"] is not None:
            h.set_shear(cell_mu=k["mu"])
    if k["c"] is not None:
        h.set_reaction(cell_c=k["c"])
    h.set_dirichlet(*args)
    return h


def assembled(problem, mesh, p, k):
    """(A csr, |A|, number of distinct values of mu or 0): the operator of the case by quadrature, scipy"""
    nvalues = 0
    if problem == "poisson":
        if k["D"] is not None:
            A, Aabs = dc.assemble(mesh, p, k["coeff"], k["D"])[:2]
        else:
            A, Aabs = pc.assemble(mesh, p, k["coeff"])[:2]
    elif k["mu"] is not None:
        A, Aabs, nvalues = sc.assemble_mu(mesh, p, k["coeff"], k["mu"])
    else:
        A, Aabs = ec.assemble(mesh, p, PI_SCALAR, k["coeff"])[:2]
    if k["c"] is not None:
        M, Mabs = rc.assemble_mass(mesh, p, k["c"], 1 if problem == "poisson" else 2)
        A, Aabs = A + M, Aabs + Mabs
    return A.tocsr(), Aabs.tocsr(), nvalues


def assembled_abs(problem, mesh, p, k):
    """|A| csr of assembled(): the same quadrature sum on the absolute values of EVERY term - the monomials c x^a y^b of
    the tabulated basis functions and the products K[X][d] dphi_X of the physical gradients included, which the |A| of
    the case modules takes after they are summed.  One entry of the matrix, unlike one entry of A u, is small enough
    for the cancellation inside those two sums to show: this is the abs-sum the count of entry_terms refers to."""
    import scipy.sparse as sp
    from dolfinx_eqlb_amd.elmtlib import polynomials as P
    from dolfinx_eqlb_amd.elmtlib.lagrange import Lagrange
    from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
    from dolfinx_eqlb_amd.eqlb.check_eqlb_conditions import cell_geometry
    import galerkin as gk
    cd, ndofs = gk.dofmap(mesh, p)
    _, detJ, K = cell_geometry(mesh)
    qp, qw = make_quadrature_triangle(2 * p + 4)
    assert np.all(qp >= 0.0)

    def ev(poly):
        out = np.zeros(qp.shape[0])
        for (a, b), c in poly.items():
            out += abs(float(c)) * qp[:, 0] ** a * qp[:, 1] ** b
        return out

    basis = Lagrange(p).basis
    phi = np.stack([ev(q) for q in basis], axis=1)                                            # [q, i]
    dphi = np.stack([np.stack([ev(P.ddx(q)), ev(P.ddy(q))], axis=1) for q in basis], axis=1)  # [q, i, X]
    g = np.einsum("cXd,qiX->cqid", np.abs(K), dphi)
    w = qw[None, :] * np.abs(detJ)[:, None]
    nc, nl = mesh.ncells, cd.shape[1]
    coeff = np.ones(nc) if k["coeff"] is None else np.abs(k["coeff"])
    if problem == "poisson":
        D = np.tile([1.0, 0.0, 1.0], (nc, 1)) if k["D"] is None else np.abs(np.asarray(k["D"]).reshape(nc, 3))
        Dm = np.stack([np.stack([D[:, 0], D[:, 1]], axis=1), np.stack([D[:, 1], D[:, 2]], axis=1)], axis=1)
        Ke = np.einsum("cq,cqid,cde,cqje->cij", w * coeff[:, None], g, Dm, g)
        bs = 1
    else:
        pi = np.full(nc, PI_SCALAR) if k["coeff"] is None else coeff
        gg = np.einsum("cq,cqid,cqjd->cij", w, g, g)
        gx = np.einsum("cq,cqir,cqjs->cirjs", w, g, g)
        Ke = np.zeros((nc, nl, 2, nl, 2))
        for r in range(2):
            Ke[:, :, r, :, r] += gg
        Ke += np.einsum("cirjs->cisjr", gx) + pi[:, None, None, None, None] * gx
        if k["mu"] is not None:
            Ke *= np.abs(k["mu"])[:, None, None, None, None]
        bs = 2
    if k["c"] is not None:
        Me = np.einsum("cq,qi,qj->cij", w * np.abs(k["c"])[:, None], phi, phi)
        if bs == 1:
            Ke = Ke + Me
        else:
            for r in range(2):
                Ke[:, :, r, :, r] += Me
    vd = (bs * cd[:, :, None] + np.arange(bs)[None, None, :]).reshape(nc, bs * nl)
    rows, cols = np.repeat(vd, bs * nl, axis=1).ravel(), np.tile(vd, (1, bs * nl)).ravel()
    return sp.csr_matrix((Ke.reshape(nc, -1).ravel(), (rows, cols)), shape=(bs * ndofs, bs * ndofs))


def _term_counts(k, nvalues):
    ts = ta = 0
    if k["D"] is not None:
        ts, ta = ts + 3, ta + 3
    if k["mu"] is not None:
        ts, ta = ts + 1, ta + nvalues
    if k["c"] is not None:
        ts, ta = ts + 1, ta + 1
    return ts, ta


def entry_terms(problem, p, valence, nq, k, nvalues=0):
    """(statement, assembled): the roundings of one entry of the matrix (the head of this file)"""
    nd = (p + 1) * (p + 2) // 2
    if problem == "poisson":
        ts, ta = pc.chain_terms(p, valence, nq)
        ts, ta = ts - nd, ta - nd * valence + 2 * nd
    else:
        ts, ta = ec.chain_terms(p, valence, nq)
        ts, ta = ts - nd, ta - 2 * nd * valence + 2 * nd
    es, ea = _term_counts(k, nvalues)
    return ts + es, ta + ea


def chain(problem, p, valence, rowlen, k):
    """c of |csr_apply(matrix, x) - apply(x)| <= c 2^-53 A (the head of this file)"""
    nd = (p + 1) * (p + 2) // 2
    es = _term_counts(k, 0)[0]
    geometry, combination = (12, 5) if problem == "poisson" else (20, 3 + 5)
    free = geometry + nd + combination + valence + es
    csr = (geometry + combination + es) + valence + (1 + rowlen)
    return free + csr


def to_scipy(m):
    import scipy.sparse as sp
    ip, ix, v = m[:3]
    n = ip.size - 1
    return sp.csr_matrix((v, ix, ip), shape=(n, n))


def eliminated_from_raw(indptr, indices, values, fixed):
    """values of P A P + (I - P) formed from the raw ones"""
    rows = np.repeat(np.arange(indptr.size - 1), np.diff(indptr))
    fx = fixed[rows] | fixed[indices]
    return np.where(fx, np.where(rows == indices, 1.0, 0.0), values)


def naive_row_sets(cell_dofs, ndofs, bs):
    """row -> set of columns, from the cells alone"""
    sets = [set() for _ in range(bs * ndofs)]
    for row in np.asarray(cell_dofs):
        cols = [bs * int(d) + s for d in row for s in range(bs)]
        for d in row:
            for r in range(bs):
                sets[bs * int(d) + r].update(cols)
    return sets
