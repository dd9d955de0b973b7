#!/usr/bin/env python3
"""primal_solve_time.py: timings of the P_p Poisson solve on the device (cpp.PrimalPoisson) at about 1M triangles.

For P_1 and P_2 on create_unit_square(N, shuffle_seed=3, perturb=0.15) (N = 500: 1,000,000 cells), f = f_ex of
tests/test_estimator_bound.py projected to DG_{p-1}, kappa = 1, Dirichlet all around:
  product    device time of one operator product y = A u, by device events around --products (>= 100) products after
             a warm-up; the byte count of a product computed from the shapes, and the achieved bytes/s against the
             measured HBM copy rate (6.29 TB/s, float4 copy)
  iteration  device time of one PCG iteration: events around a solve of exactly --iterations iterations (rtol = 0)
  zero       iterations and time to rtol 1e-8 from u = 0
  prolonged  the same mesh refined at 2 % of its cells (fixed seed) on the device: iterations and time to rtol 1e-8 from
             zero and from the prolonged solution of the unrefined mesh
  host       scipy.sparse.linalg.cg with the same diagonal preconditioner and tolerance on the matrix assembled from the
             same tables, and spsolve, on the host of the same machine (--host; each under a time budget, reported as
             "not finished" beyond it)
  --elasticity  after the Poisson figures, the same figures for the P_p^2 elasticity solve (cpp.PrimalElasticity): pi_1 = 1,
             u = 0 all around in both rows, the body force (f_ex, f_ex(y, x)); vectors have 2 ndofs rows, the solution
             is prolonged with bs = 2, and the product time is also given as a multiple of Poisson's at the same degree
  --multilevel  instead of the figures above: a hierarchy by uniform marking on the device from create_unit_square(
             --coarse-n) up to within 10 % of 1M triangles (every level has four times the cells), one solver handle per
             level, and for every degree (with --elasticity also for the elasticity solve) the device time of one
             application of the multilevel preconditioner (cpp.Multilevel.precondition_raw), of one iteration, the
             iterations and the time to rtol 1e-8 from zero of the Jacobi entry and of the hierarchy in the same process,
             and an estimate of the launch share of an application: the time per launch of an application on the
             coarsest levels alone (up to 4 096 cells: nothing but launches), times the launches of the full one
  --nrhs R ...  instead of the figures above, on the hierarchy of --multilevel (9 levels, 1M triangles): several right-hand
             sides in one call against one call per right-hand side, in one process and on the same handles.  For every
             degree, for the Jacobi entry (cpp.PrimalPoisson) and the hierarchy entry (cpp.Multilevel) and for every
             R given: R calls of solve_raw - the only way before the *_many entries, which they leave alone - against
             one solve_many_raw of the same R systems (b_c = (1 + c / 2) b plus 1 % noise of its own, rtol 1e-8 from
             zero).  Each pair is repeated --repeats (>= 5) times after clock-settle probes as bench.py runs them
             (repeated for at least 40 ms and until two agree within 1 %, at most 24); median and spread (max - min)
             of the wall time of the calls, which wait for the device, are printed, and whether the gain of the
             many-solve exceeds the spread of the R single calls
  --reaction  instead of the figures above: the reaction term + c u of set_reaction.  (1) At --n, for every degree (with
             --elasticity also for the elasticity product): one masked product without and with the term (a cell-wise c,
             uniform in [0, 1000]) ON THE SAME HANDLE in one process, switched by set_reaction: after clock-settle
             probes, --repeats (>= 5) alternating blocks of --products products each; median and spread (max - min) of
             the time per product, and whether the difference exceeds the spread.  With --plain-only the blocks without
             the term alone: the figure of the same-call A/B against the parent commit (tools/build_head.sh,
             tools/run_variants.sh).  (2) On the hierarchy of --multilevel, Poisson: one implicit heat step, c = 1 / tau
             on every level for every tau of --taus (1e-2 and 1e-4) next to c = 0: iterations and time to rtol 1e-8 from zero of the
             Jacobi entry, of the hierarchy, and of the hierarchy with local smoothing and the exact coarse solve
             (factored again after every change of c).  One run each
  --diffusion  instead of the figures above: the cell-wise diffusion tensor of set_diffusion (Poisson only; random rotations
             of diag(1, 1e-2)).  At --n, for every degree: the masked product without and with the tensor ON THE SAME
             HANDLE in one process, switched by set_diffusion; primal_flux_dg of degree p - 1 against
             primal_flux_dg_tensor; cell_sig2 of estimate at k = p against the weighted entry.  Medians of --repeats
             blocks of --products calls, the spread beside them.  With --plain-only the product without the term alone
             (runs on a library without the term too: EQLB_AMD_LIB, for an A/B against another build in one session).
  --shear    instead of the figures above: the cell-wise shear modulus of set_shear (elasticity only).  (1) At --n, for every
             degree: one masked elasticity product without and with the term (a cell-wise mu, log-uniform in [1e-3, 1e3])
             ON THE SAME HANDLE in one process, switched by set_shear, and primal_stress_dg_mu (degree p - 1, the same mu)
             against primal_stress_dg: after clock-settle probes, --repeats (>= 5) alternating blocks of --products calls
             each; median and spread (max - min) of the time per call, and whether the difference exceeds the spread.
             (2) With --multilevel: mu = the contrast on the cells of the coarsest mesh whose centroid lies right of
             x = 1/2 and on their descendants, mu = 1 on the others, pi_1 = 1, for the contrasts 1, 10 and 1000, on the nine uniform levels of --multilevel and on an adaptive hierarchy
             (create_unit_square(16), ten steps that refine the cells with a vertex on the interface; mu crosses the
             refinements through prolong_dg): iterations and time to rtol 1e-8 from zero of the Jacobi entry, of the
             hierarchy, and (adaptive) of the hierarchy with local smoothing and the exact coarse solve.  One run each
  --check-every LIB:N ...   the PCG of P_2 to rtol 1e-8 from zero once per library (builds of libeqlb_amd.so with
             -DEQLB_PRIMAL_CHECK_EVERY=N, tools/build_variant.sh NAME "-D..." eqlb_primal_solve), each in a child process
Prints one line per figure and, last, one JSON line with all of them.  Nothing here is a pass/fail condition.
"""

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

HBM_COPY_RATE = 6.29e12   # bytes/s, measured float4 copy on the MI355X


def say(*a):
    print(*a, flush=True)


def f_ex(x, y):
    s, c = np.sin, np.cos
    return 2 * np.pi ** 2 * s(np.pi * x) * s(np.pi * y) * (1 + x) - 2 * np.pi * c(np.pi * x) * s(np.pi * y)


def rhs_dg(mesh, d, swap=False):
    """f_ex interpolated at the DG_d nodes (nodal values [ncells * nd_d]); swap: f_ex(y, x)"""
    from dolfinx_eqlb_amd.elmtlib.lagrange import lagrange_nodes
    X = np.array([[float(a), float(b)] for a, b in lagrange_nodes(d)])
    xc = mesh.x[mesh.cell_nodes, :2]
    pts = xc[:, None, 0, :] + X[None, :, 0:1] * (xc[:, 1] - xc[:, 0])[:, None, :] \
        + X[None, :, 1:2] * (xc[:, 2] - xc[:, 0])[:, None, :]
    return np.ascontiguousarray(f_ex(pts[..., 1 if swap else 0], pts[..., 0 if swap else 1]).ravel())


def product_bytes(mesh, p, bs=1):
    """compulsory bytes of one product from the shapes: the cell pass reads the dofmap, cellJ and u once and writes
    y_loc; the sum pass reads y_loc, the slot lists, the two offset tables and the mask and writes y.  bs components
    per DOF (elasticity: 2): u, y_loc, the mask and y grow by bs, the dofmap, cellJ and the lists do not.  Returns the
    bytes and the number of rows bs * ndofs"""
    nd, ne = (p + 1) * (p + 2) // 2, p - 1
    nc, nn, nf = mesh.ncells, mesh.nnodes, mesh.nfacets
    ndofs = nn + nf * ne + nc * (p - 1) * (p - 2) // 2
    cell = nc * nd * 4 + nc * 32 + bs * ndofs * 8 + bs * nc * nd * 8
    gather = bs * nc * nd * 8 + 3 * nc * (1 + ne) * 4 + (nn + nf + 2) * 4 + bs * ndofs + bs * ndofs * 8
    return cell + gather, bs * ndofs


def timed_solve(torch, h, b, u0, rtol, maxit):
    """(info, device ms) of one solve from u0 (copied), events around it"""
    u = u0.clone()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    info = h.solve_raw(b.data_ptr(), u.data_ptr(), rtol, 0.0, maxit)
    e1.record()
    torch.cuda.synchronize()
    return info, e0.elapsed_time(e1), u


def make_problem(cpp, torch, dm, p, elasticity=False):
    mesh = dm.mesh
    if elasticity:
        h = cpp.PrimalElasticity(dm, p, 1.0)
        h.set_dirichlet(mesh.boundary_facets(), mesh.boundary_facets())
        f = torch.from_numpy(np.stack([rhs_dg(mesh, p - 1), rhs_dg(mesh, p - 1, swap=True)])).cuda()
    else:
        h = cpp.PrimalPoisson(dm, p)
        h.set_dirichlet(mesh.boundary_facets())
        f = torch.from_numpy(rhs_dg(mesh, p - 1)).cuda()
    b = torch.zeros((2 if elasticity else 1) * h.ndofs, dtype=torch.float64, device="cuda")
    h.load_raw(p - 1, f.data_ptr(), None, b.data_ptr())
    torch.cuda.synchronize()
    return h, b


def host_matrix_elasticity(mesh, p):
    """A (csr, blocked rows 2 dof + r) of the elasticity problem with pi_1 = 1 from the statement's tables, and the free
    rows: per cell adet (delta_rs (D_00 + D_11) + D_sr + D_rs)[i][j] with D_ab = sum_XY K[X][a] K[Y][b] M_XY"""
    import scipy.sparse as sp
    from dolfinx_eqlb_amd.lsolver import primal
    from dolfinx_eqlb_amd.mesh.transfer import lagrange_dofmap
    cd, ndofs = lagrange_dofmap(mesh, p)
    x, cn = mesh.x, mesh.cell_nodes
    J00, J01 = x[cn[:, 1], 0] - x[cn[:, 0], 0], x[cn[:, 2], 0] - x[cn[:, 0], 0]
    J10, J11 = x[cn[:, 1], 1] - x[cn[:, 0], 1], x[cn[:, 2], 1] - x[cn[:, 0], 1]
    det = J00 * J11 - J01 * J10
    K = ((J11 / det, -J01 / det), (-J10 / det, J00 / det))
    S, Cx = primal.stiffness_table(p), primal.cross_table(p)
    M = ((S[0], Cx), (Cx.T, S[2]))
    D = [[sum((K[X][a] * K[Y][b])[:, None, None] * M[X][Y][None] for X in range(2) for Y in range(2))
          for b in range(2)] for a in range(2)]
    nl = cd.shape[1]
    Ke = np.zeros((mesh.ncells, nl, 2, nl, 2))
    for r in range(2):
        Ke[:, :, r, :, r] += D[0][0] + D[1][1]
        for c in range(2):
            Ke[:, :, r, :, c] += D[c][r] + D[r][c]
    Ke *= np.abs(det)[:, None, None, None, None]
    vd = (2 * cd[:, :, None] + np.arange(2)[None, None, :]).reshape(mesh.ncells, 2 * nl)
    A = sp.csr_matrix((Ke.ravel(), (np.repeat(vd, 2 * nl, axis=1).ravel(), np.tile(vd, (1, 2 * nl)).ravel())),
                      shape=(2 * ndofs, 2 * ndofs))
    fixed = np.repeat(primal.dirichlet_mask(mesh, p, mesh.boundary_facets()), 2)
    return A, np.nonzero(~fixed)[0]


def host_matrix(mesh, p):
    """A (csr) from the statement's tables, the free rows, in the handle's numbering"""
    import scipy.sparse as sp
    from dolfinx_eqlb_amd.lsolver import primal
    from dolfinx_eqlb_amd.mesh.transfer import lagrange_dofmap
    cd, ndofs = lagrange_dofmap(mesh, p)
    x, cn = mesh.x, mesh.cell_nodes
    J00, J01 = x[cn[:, 1], 0] - x[cn[:, 0], 0], x[cn[:, 2], 0] - x[cn[:, 0], 0]
    J10, J11 = x[cn[:, 1], 1] - x[cn[:, 0], 1], x[cn[:, 2], 1] - x[cn[:, 0], 1]
    det = J00 * J11 - J01 * J10
    K00, K01, K10, K11 = J11 / det, -J01 / det, -J10 / det, J00 / det
    C = (K00 * K00 + K01 * K01, K00 * K10 + K01 * K11, K10 * K10 + K11 * K11)
    S = primal.stiffness_table(p)
    Ke = np.abs(det)[:, None, None] * sum(C[m][:, None, None] * S[m][None] for m in range(3))
    nl = cd.shape[1]
    A = sp.csr_matrix((Ke.ravel(), (np.repeat(cd, nl, axis=1).ravel(), np.tile(cd, (1, nl)).ravel())),
                      shape=(ndofs, ndofs))
    fixed = primal.dirichlet_mask(mesh, p, mesh.boundary_facets())
    return A, np.nonzero(~fixed)[0]


def host_figures(mesh, p, b, budget, direct, elasticity=False):
    import scipy.sparse.linalg as spla
    out = {}
    t0 = time.perf_counter()
    A, free = host_matrix_elasticity(mesh, p) if elasticity else host_matrix(mesh, p)
    Aff = A[free][:, free].tocsr()
    bf = b[free]
    out["assemble_s"] = time.perf_counter() - t0
    say(f"  host: assembled {Aff.shape[0]} free rows in {out['assemble_s']:.1f} s")
    dinv = 1.0 / Aff.diagonal()
    M = spla.LinearOperator(Aff.shape, matvec=lambda v: dinv * v)
    n = [0]
    t0 = time.perf_counter()

    class Budget(Exception):
        pass

    def cb(_):
        n[0] += 1
        if time.perf_counter() - t0 > budget:
            raise Budget()

    try:
        _, flag = spla.cg(Aff, bf, rtol=1e-8, atol=0.0, M=M, maxiter=200000, callback=cb)
        out["cg"] = dict(iterations=n[0], seconds=time.perf_counter() - t0, converged=int(flag == 0))
    except Budget:
        out["cg"] = dict(iterations=n[0], seconds=time.perf_counter() - t0, converged=0, note="not finished")
    say(f"  host: scipy cg (Jacobi, rtol 1e-8): {out['cg']}")
    if not direct:
        say("  host: spsolve not measured at this degree (--spsolve-degrees)")
        return out
    t0 = time.perf_counter()
    spla.spsolve(Aff.tocsc(), bf)
    out["spsolve_s"] = time.perf_counter() - t0
    say(f"  host: spsolve {out['spsolve_s']:.1f} s")
    return out


def run_degree(args, cpp, torch, dm, p, res, elasticity=False):
    """the figures of one degree; with elasticity the name of the degree is E_p and ndofs counts the 2 ndofs rows"""
    mesh = dm.mesh
    bs, P = (2, "E") if elasticity else (1, "P")
    h, b = make_problem(cpp, torch, dm, p, elasticity)
    nbytes, ndofs = product_bytes(mesh, p, bs)
    r = dict(ncells=mesh.ncells, ndofs=ndofs, product_bytes=nbytes)
    u = torch.from_numpy(np.random.default_rng(0).standard_normal(ndofs)).cuda()
    y = torch.empty_like(u)
    for _ in range(10):
        h.apply_raw(u.data_ptr(), y.data_ptr(), True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.products):
        h.apply_raw(u.data_ptr(), y.data_ptr(), True)
    e1.record()
    torch.cuda.synchronize()
    r["product_ms"] = e0.elapsed_time(e1) / args.products
    r["product_bytes_per_s"] = nbytes / (r["product_ms"] * 1e-3)
    r["product_fraction_of_copy_rate"] = r["product_bytes_per_s"] / HBM_COPY_RATE
    say(f"{P}_{p}: {mesh.ncells} cells, {ndofs} DOFs; product {r['product_ms']:.4f} ms over {args.products} products, "
        f"{nbytes / 1e6:.1f} MB -> {r['product_bytes_per_s'] / 1e12:.3f} TB/s = "
        f"{100 * r['product_fraction_of_copy_rate']:.1f} % of the copy rate")
    if elasticity and f"P{p}" in res:
        r["product_over_poisson"] = r["product_ms"] / res[f"P{p}"]["product_ms"]
        say(f"E_{p}: product = {r['product_over_poisson']:.2f} x the Poisson product (expected between 1 and about 2.7: "
            f"twice the vector data against 8 contractions for 3)")
    zero = torch.zeros(ndofs, dtype=torch.float64, device="cuda")
    timed_solve(torch, h, b, zero, 0.0, 20)   # warm-up
    info, ms, _ = timed_solve(torch, h, b, zero, 0.0, args.iterations)
    r["iteration_ms"] = ms / max(info["iterations"], 1)
    say(f"{P}_{p}: PCG iteration {r['iteration_ms']:.4f} ms ({info['iterations']} iterations in {ms:.1f} ms)")
    info, ms, usol = timed_solve(torch, h, b, zero, 1e-8, args.maxit)
    r["zero"] = dict(iterations=info["iterations"], ms=ms, converged=info["converged"],
                     replacements=info["replacements"])
    say(f"{P}_{p}: to rtol 1e-8 from zero: {r['zero']}")
    if args.check_only:
        res[f"{P}{p}"] = r
        return
    # 2 % refinement on the device, the solution prolonged
    marked = np.random.default_rng(42).choice(mesh.ncells, size=mesh.ncells // 50, replace=False).astype(np.int32)
    ref = dm.refine(np.sort(marked), keep_plan=True)
    h2, b2 = make_problem(cpp, torch, ref.dmesh, p, elasticity)
    u2 = ref.prolong(p, usol, bs=bs).reshape(-1)
    # the prolonged values of the boundary DOFs are the (zero) Dirichlet values of the new mesh
    zero2 = torch.zeros(bs * h2.ndofs, dtype=torch.float64, device="cuda")
    i0, ms0, _ = timed_solve(torch, h2, b2, zero2, 1e-8, args.maxit)
    i1, ms1, _ = timed_solve(torch, h2, b2, u2, 1e-8, args.maxit)
    r["refined"] = dict(ncells=ref.dmesh.mesh.ncells, ndofs=bs * h2.ndofs,
                        zero=dict(iterations=i0["iterations"], ms=ms0, converged=i0["converged"]),
                        prolonged=dict(iterations=i1["iterations"], ms=ms1, converged=i1["converged"]))
    say(f"{P}_{p}: refined at 2 % ({r['refined']['ncells']} cells): from zero {r['refined']['zero']}, "
        f"from the prolonged solution {r['refined']['prolonged']}")
    ref.close()
    if args.host:
        r["host"] = host_figures(mesh, p, b.cpu().numpy(), args.host_budget, p in args.spsolve_degrees, elasticity)
    res[f"{P}{p}"] = r


def timed_calls(torch, fn, n):
    """device ms per call of fn, by events around n calls after a warm-up of 5"""
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def settle_probes(fn):
    """untimed calls of fn for at least 40 ms and until two agree within 1 % (at most 24): the clocks after the idle
    set-up, as bench.py settles them; returns the probe times in ms"""
    probes, t0 = [], time.perf_counter()
    while len(probes) < 24:
        tp = time.perf_counter()
        fn()
        probes.append((time.perf_counter() - tp) * 1e3)
        if len(probes) >= 2 and (time.perf_counter() - t0) * 1e3 >= 40.0 \
                and abs(probes[-1] - probes[-2]) <= 0.01 * probes[-2]:
            break
    return probes


def device_hierarchy(args, cpp):
    """the levels of --multilevel: (DeviceMesh per level, Refinement per link, cells per level)"""
    from dolfinx_eqlb_amd.mesh import create_unit_square
    base = create_unit_square(args.coarse_n, shuffle_seed=3, perturb=0.15)
    L = max(1, int(round(np.log(1.0e6 / base.ncells) / np.log(4.0))))
    if abs(base.ncells * 4 ** L - 1.0e6) > 1.0e5:
        say(f"--coarse-n {args.coarse_n}: {base.ncells * 4 ** L} cells on level {L} are not within 10 % of 1M triangles")
        sys.exit(1)
    t0 = time.perf_counter()
    dms, refs = [cpp.DeviceMesh(base)], []
    for _ in range(L):
        refs.append(dms[-1].refine(np.arange(dms[-1].mesh.ncells, dtype=np.int32), keep_plan=True))
        dms.append(refs[-1].dmesh)
    cells = [d.mesh.ncells for d in dms]
    say(f"hierarchy: {L + 1} levels, cells {cells} in {time.perf_counter() - t0:.1f} s")
    return dms, refs, cells


def run_many(args, cpp, torch, res):
    """the figures of --nrhs"""
    dms, refs, cells = device_hierarchy(args, cpp)
    L = len(refs)
    rmax = max(args.nrhs)
    for p in args.degrees:
        hs = []
        for dm in dms[:-1]:
            hs.append(cpp.PrimalPoisson(dm, p))
            hs[-1].set_dirichlet(dm.mesh.boundary_facets())
        top, b = make_problem(cpp, torch, dms[-1], p)
        hs.append(top)
        ml = cpp.Multilevel(hs, refs)
        n = top.ndofs
        gen = torch.Generator(device="cuda").manual_seed(p)
        B = torch.stack([(1.0 + 0.5 * c) * b + 0.01 * b.abs().max()
                         * torch.randn(n, dtype=torch.float64, device="cuda", generator=gen) for c in range(rmax)])
        U = torch.zeros_like(B)
        for name, h in (("jacobi", top), ("hierarchy", ml)):
            for R in args.nrhs:
                def singles():
                    U.zero_()
                    return [h.solve_raw(B[c].data_ptr(), U[c].data_ptr(), 1e-8, 0.0, args.maxit) for c in range(R)]

                def many():
                    U.zero_()
                    return h.solve_many_raw(R, B.data_ptr(), U.data_ptr(), 1e-8, 0.0, args.maxit)

                i_single, x_single = singles(), U[:R].clone()
                i_many, x_many = many(), U[:R].clone()
                same = bool(torch.equal(x_single.view(torch.int64), x_many.view(torch.int64))) and i_single == i_many
                probes = settle_probes(many)
                t_single, t_many = [], []
                for _ in range(args.repeats):
                    for fn, out in ((singles, t_single), (many, t_many)):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        out.append((time.perf_counter() - t0) * 1e3)
                ms, mm = float(np.median(t_single)), float(np.median(t_many))
                ss, sm = float(np.ptp(t_single)), float(np.ptp(t_many))
                r = dict(levels=L + 1, cells=cells[-1], ndofs=n, nrhs=R, repeats=args.repeats,
                         iterations=[i["iterations"] for i in i_many], converged=[i["converged"] for i in i_many],
                         same_bits_and_info=same, settle_probes=len(probes),
                         single_ms=dict(median=ms, spread=ss, all=t_single),
                         many_ms=dict(median=mm, spread=sm, all=t_many), ratio=mm / ms,
                         gain_exceeds_spread=bool(ms - mm > ss))
                res[f"MANY_{name}_P{p}_R{R}"] = r
                say(f"P_{p} {name} R = {R}: {R} x solve {ms:.2f} ms (spread {ss:.2f}), 1 x solve_many {mm:.2f} ms "
                    f"(spread {sm:.2f}) = {mm / ms:.3f} of it over {args.repeats} repeats after {len(probes)} probes; "
                    f"iterations {r['iterations']}; same bits and info: {same}; gain exceeds the spread of the single "
                    f"calls: {r['gain_exceeds_spread']}")
        ml.close()


def run_multilevel(args, cpp, torch, res):
    """the figures of --multilevel"""
    dms, refs, cells = device_hierarchy(args, cpp)
    L = len(refs)
    small =max(2, sum(1 for c in cells if c <= 4096))   # levels of the launch-bound sub-hierarchy
    for elasticity in ([False, True] if args.elasticity else [False]):
        bs, P = (2, "E") if elasticity else (1, "P")
        for p in args.degrees:
            hs = []
            for dm in dms[:-1]:
                bf = dm.mesh.boundary_facets()
                hs.append(cpp.PrimalElasticity(dm, p, 1.0) if elasticity else cpp.PrimalPoisson(dm, p))
                hs[-1].set_dirichlet(*([bf, bf] if elasticity else [bf]))
            top, b = make_problem(cpp, torch, dms[-1], p, elasticity)
            hs.append(top)
            ml = cpp.Multilevel(hs, refs)
            n = bs * top.ndofs
            r = dict(levels=L + 1, cells=cells, ndofs=n)
            x = torch.from_numpy(np.random.default_rng(0).standard_normal(n)).cuda()
            z = torch.empty_like(x)
            r["precondition_ms"] = timed_calls(torch, lambda: ml.precondition_raw(x.data_ptr(), z.data_ptr()),
                                               args.products)
            mls = cpp.Multilevel(hs[:small], refs[:small - 1])
            ns = bs * hs[small - 1].ndofs
            xs, zs = x[:ns].clone(), z[:ns].clone()
            per_launch = timed_calls(torch, lambda: mls.precondition_raw(xs.data_ptr(), zs.data_ptr()),
                                     args.products) / (2 + 4 * (small - 1))
            mls.close()
            r["launches"] = 2 + 4 * L
            r["launch_ms"] = per_launch
            r["launch_share"] = min(1.0, r["launches"] * per_launch / r["precondition_ms"])
            say(f"{P}_{p}: {n} rows; one application {r['precondition_ms']:.4f} ms over {args.products} applications, "
                f"{r['launches']} launches of about {1e3 * per_launch:.1f} us each (measured on the {small} coarsest "
                f"levels): launch share about {100 * r['launch_share']:.0f} %")
            zero = torch.zeros(n, dtype=torch.float64, device="cuda")
            timed_solve(torch, ml, b, zero, 0.0, 8)   # warm-up
            info, ms, _ = timed_solve(torch, ml, b, zero, 0.0, args.iterations)
            r["iteration_ms"] = ms / max(info["iterations"], 1)
            say(f"{P}_{p}: iteration with the hierarchy {r['iteration_ms']:.4f} ms ({info['iterations']} iterations in "
                f"{ms:.1f} ms)")
            info, ms, _ = timed_solve(torch, top, b, zero, 0.0, args.iterations)
            r["jacobi_iteration_ms"] = ms / max(info["iterations"], 1)
            for name, h in (("jacobi", top), ("hierarchy", ml)):
                info, ms, _ = timed_solve(torch, h, b, zero, 1e-8, args.maxit)
                r[name] = dict(iterations=info["iterations"], ms=ms, converged=info["converged"],
                               replacements=info["replacements"], breakdown=info["breakdown"])
                say(f"{P}_{p}: {name} to rtol 1e-8 from zero: {r[name]}")
            r["speedup"] = r["jacobi"]["ms"] / r["hierarchy"]["ms"]
            say(f"{P}_{p}: Jacobi iteration {r['jacobi_iteration_ms']:.4f} ms; the hierarchy solves in "
                f"1 / {r['speedup']:.2f} of the time of Jacobi")
            ml.close()
            res[f"ML_{P}{p}"] = r


def run_reaction(args, cpp, torch, res):
    """the figures of --reaction"""
    from dolfinx_eqlb_amd.mesh import create_unit_square
    dm = cpp.DeviceMesh(create_unit_square(args.n, shuffle_seed=3, perturb=0.15))
    nc = dm.mesh.ncells
    cc = 1000.0 * torch.rand(nc, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    for elasticity in ([False, True] if args.elasticity else [False]):
        bs, P = (2, "E") if elasticity else (1, "P")
        for p in args.degrees:
            h, _ = make_problem(cpp, torch, dm, p, elasticity)
            n = bs * h.ndofs
            x = torch.from_numpy(np.random.default_rng(0).standard_normal(n)).cuda()
            y = torch.empty_like(x)

            def product():
                h.apply_raw(x.data_ptr(), y.data_ptr(), True)

            def probe():
                product()
                torch.cuda.synchronize()

            states = ("off",) if args.plain_only else ("off", "on")
            probes = settle_probes(probe)
            t = {s: [] for s in states}
            for _ in range(args.repeats):
                for s in states:
                    if not args.plain_only:
                        h.set_reaction_raw(0.0, cc.data_ptr() if s == "on" else None)
                    t[s].append(timed_calls(torch, product, args.products))
            r = dict(cells=nc, rows=n, products=args.products, repeats=args.repeats, settle_probes=len(probes))
            for s in states:
                r[s] = dict(median_ms=float(np.median(t[s])), spread_ms=float(np.ptp(t[s])), all_ms=t[s])
            line = f"{P}_{p}: {n} rows; product without the term {r['off']['median_ms']:.4f} ms (spread " \
                   f"{r['off']['spread_ms']:.4f})"
            if not args.plain_only:
                diff = r["on"]["median_ms"] - r["off"]["median_ms"]
                r["ratio"] = r["on"]["median_ms"] / r["off"]["median_ms"]
                r["difference_exceeds_spread"] = bool(abs(diff) > max(r["on"]["spread_ms"], r["off"]["spread_ms"]))
                line += f", with it {r['on']['median_ms']:.4f} ms (spread {r['on']['spread_ms']:.4f}) = {r['ratio']:.3f} " \
                        f"of it; the difference exceeds the spread: {r['difference_exceeds_spread']}"
            say(line + f"; median of {args.repeats} blocks of {args.products} products after {len(probes)} probes")
            res[f"REACTION_PRODUCT_{P}{p}"] = r
            h.close()
    if args.plain_only or not args.multilevel:
        return
    dms, refs, cells = device_hierarchy(args, cpp)
    for p in args.degrees:
        hs = []
        for d in dms[:-1]:
            hs.append(cpp.PrimalPoisson(d, p))
            hs[-1].set_dirichlet(d.mesh.boundary_facets())
        top, b = make_problem(cpp, torch, dms[-1], p)
        hs.append(top)
        ml = cpp.Multilevel(hs, refs)
        mlc = cpp.Multilevel(hs, refs, local=True, coarse=True)
        zero = torch.zeros(top.ndofs, dtype=torch.float64, device="cuda")
        for tau in [None] + list(args.taus):
            for h in hs:
                h.set_reaction(0.0 if tau is None else 1.0 / tau)
            mlc.set_coarse(True)     # (the factor is a snapshot of the operator of level 0)
            r = dict(levels=len(dms), cells=cells[-1], ndofs=top.ndofs, c=0.0 if tau is None else 1.0 / tau)
            for name, h in (("jacobi", top), ("hierarchy", ml), ("local_coarse", mlc)):
                info, ms, _ = timed_solve(torch, h, b, zero, 1e-8, args.maxit)
                r[name] = dict(iterations=info["iterations"], ms=ms, converged=info["converged"],
                               breakdown=info["breakdown"])
            say(f"P_{p} heat step tau = {tau}: " + "; ".join(
                f"{name} {r[name]['iterations']} iterations in {r[name]['ms']:.1f} ms"
                for name in ("jacobi", "hierarchy", "local_coarse")) + " (one run each)")
            res[f"HEAT_P{p}_tau{tau}"] = r
        ml.close()
        mlc.close()


def on_off_blocks(args, torch, fns, probe):
    """median, spread and all block times per state of fns = {state: (prepare, call)}; the states are off and on"""
    probes = settle_probes(probe)
    t = {s_: [] for s_ in fns}
    for _ in range(args.repeats):
        for s_, (prepare, call) in fns.items():
            prepare()
            t[s_].append(timed_calls(torch, call, args.products))
    r = dict(products=args.products, repeats=args.repeats, settle_probes=len(probes))
    for s_ in fns:
        r[s_] = dict(median_ms=float(np.median(t[s_])), spread_ms=float(np.ptp(t[s_])), all_ms=t[s_])
    r["ratio"] = r["on"]["median_ms"] / r["off"]["median_ms"]
    diff = r["on"]["median_ms"] - r["off"]["median_ms"]
    r["difference_exceeds_spread"] = bool(abs(diff) > max(r["on"]["spread_ms"], r["off"]["spread_ms"]))
    return r


def on_off_line(args, r):
    return (f" without the term {r['off']['median_ms']:.4f} ms (spread {r['off']['spread_ms']:.4f}), with it "
            f"{r['on']['median_ms']:.4f} ms (spread {r['on']['spread_ms']:.4f}) = {r['ratio']:.3f} of it; the "
            f"difference exceeds the spread: {r['difference_exceeds_spread']}; median of {args.repeats} blocks of "
            f"{args.products} calls after {r['settle_probes']} probes")


def run_diffusion(args, cpp, torch, res):
    """the figures of --diffusion"""
    from dolfinx_eqlb_amd.mesh import create_unit_square
    dm = cpp.DeviceMesh(create_unit_square(args.n, shuffle_seed=3, perturb=0.15))
    nc = dm.mesh.ncells
    gen = torch.Generator(device="cuda").manual_seed(1)
    th = np.pi * torch.rand(nc, dtype=torch.float64, device="cuda", generator=gen)
    c, s_, eps = torch.cos(th), torch.sin(th), 1e-2
    D = torch.stack([c * c + eps * s_ * s_, c * s_ * (1.0 - eps), s_ * s_ + eps * c * c], dim=1).contiguous()
    for p in args.degrees:
        h, _ = make_problem(cpp, torch, dm, p)
        n = h.ndofs
        x = torch.from_numpy(np.random.default_rng(0).standard_normal(n)).cuda()
        y = torch.empty_like(x)

        def product():
            h.apply_raw(x.data_ptr(), y.data_ptr(), True)

        def probe():
            product()
            torch.cuda.synchronize()

        if args.plain_only:
            probes = settle_probes(probe)
            t = [timed_calls(torch, product, args.products) for _ in range(args.repeats)]
            r = dict(cells=nc, rows=n, products=args.products, repeats=args.repeats, settle_probes=len(probes),
                     off=dict(median_ms=float(np.median(t)), spread_ms=float(np.ptp(t)), all_ms=t))
            say(f"P_{p}: {n} rows; product without the term {r['off']['median_ms']:.4f} ms (spread "
                f"{r['off']['spread_ms']:.4f}); median of {args.repeats} blocks of {args.products} products after "
                f"{len(probes)} probes")
            res[f"DIFFUSION_PRODUCT_P{p}"] = r
            h.close()
            continue
        r = on_off_blocks(args, torch, {"off": (lambda: h.set_diffusion_raw(None), product),
                                        "on": (lambda: h.set_diffusion_raw(D.data_ptr()), product)}, probe)
        r.update(cells=nc, rows=n)
        say(f"P_{p}: {n} rows; product" + on_off_line(args, r))
        res[f"DIFFUSION_PRODUCT_P{p}"] = r
        h.close()
        # the projected flux of degree p - 1
        cd, ndofs = dm.lagrange_dofmap(p, device=True)
        d = p - 1
        nd = (d + 1) * (d + 2) // 2
        G = torch.empty(nc * nd * 2, dtype=torch.float64, device="cuda")

        def plain():
            cpp.primal_flux_dg_raw(dm, p, d, 1, cd.data_ptr(), ndofs, x.data_ptr(), None, G.data_ptr())

        def tensor():
            cpp.primal_flux_dg_tensor_raw(dm, p, d, 1, cd.data_ptr(), ndofs, x.data_ptr(), None, D.data_ptr(), G.data_ptr())

        def probe_flux():
            plain()
            torch.cuda.synchronize()

        r = on_off_blocks(args, torch, {"off": (lambda: None, plain), "on": (lambda: None, tensor)}, probe_flux)
        r.update(cells=nc, degree_dg=d)
        say(f"P_{p}: primal_flux_dg of degree {d}" + on_off_line(args, r))
        res[f"DIFFUSION_FLUX_P{p}"] = r
        # the flux norm of the estimator at k = p with DG_{k-1} data (every call waits for the device by itself)
        k = p
        xe = torch.from_numpy(np.random.default_rng(1).standard_normal(nc * k * (k + 2))).cuda()
        fe = torch.from_numpy(np.random.default_rng(2).standard_normal(nc * nd)).cuda()
        sig = torch.empty(nc, dtype=torch.float64, device="cuda")
        tensor()

        def est_plain():
            cpp.estimate_raw(dm, k, 1, xe.data_ptr(), G.data_ptr(), fe.data_ptr(), None, sig.data_ptr(), None,
                             degree_dg=d)

        def est_weighted():
            cpp.estimate_weighted_raw(dm, k, d, 1, xe.data_ptr(), G.data_ptr(), fe.data_ptr(), None, D.data_ptr(), None,
                                      sig.data_ptr(), None)

        r = on_off_blocks(args, torch, {"off": (lambda: None, est_plain), "on": (lambda: None, est_weighted)}, est_plain)
        r.update(cells=nc, k=k, degree_dg=d)
        say(f"RT_{k}: cell_sig2 of the estimate" + on_off_line(args, r))
        res[f"DIFFUSION_ESTIMATE_K{k}"] = r


def run_shear(args, cpp, torch, res):
    """the figures of --shear"""
    from dolfinx_eqlb_amd.mesh import create_unit_square
    dm = cpp.DeviceMesh(create_unit_square(args.n, shuffle_seed=3, perturb=0.15))
    nc = dm.mesh.ncells
    gen = torch.Generator(device="cuda").manual_seed(1)
    mu = 10.0 ** (-3.0 + 6.0 * torch.rand(nc, dtype=torch.float64, device="cuda", generator=gen))

    def blocks(fns, probe):
        return on_off_blocks(args, torch, fns, probe)

    def line(what, r):
        return what + on_off_line(args, r)[1:]

    for p in args.degrees:
        h, _ = make_problem(cpp, torch, dm, p, True)
        n = 2 * h.ndofs
        x = torch.from_numpy(np.random.default_rng(0).standard_normal(n)).cuda()
        y = torch.empty_like(x)

        def product():
            h.apply_raw(x.data_ptr(), y.data_ptr(), True)

        def probe():
            product()
            torch.cuda.synchronize()

        r = blocks({"off": (lambda: h.set_shear_raw(1.0, None), product),
                    "on": (lambda: h.set_shear_raw(1.0, mu.data_ptr()), product)}, probe)
        r.update(cells=nc, rows=n)
        say(f"E_{p}: {n} rows; product " + line("", r))
        res[f"SHEAR_PRODUCT_E{p}"] = r
        h.close()
        # the projected stress of degree p - 1
        cd, ndofs = dm.lagrange_dofmap(p, device=True)
        d = p - 1
        out = torch.empty(2 * nc * (d + 1) * (d + 2), dtype=torch.float64, device="cuda")
        u = x[:2 * ndofs]

        def plain():
            cpp.primal_stress_dg_raw(dm, p, d, cd.data_ptr(), ndofs, u.data_ptr(), 1.0, None, out.data_ptr())

        def with_mu():
            cpp.primal_stress_dg_mu_raw(dm, p, d, cd.data_ptr(), ndofs, u.data_ptr(), 1.0, None, 1.0, mu.data_ptr(),
                                        out.data_ptr())

        def probe_stress():
            plain()
            torch.cuda.synchronize()

        r = blocks({"off": (lambda: None, plain), "on": (lambda: None, with_mu)}, probe_stress)
        r.update(cells=nc, degree_dg=d)
        say(f"E_{p}: primal_stress_dg of degree {d} " + line("", r))
        res[f"SHEAR_STRESS_E{p}"] = r
    if not args.multilevel:
        return

    def right_of(mesh):
        return (mesh.x[mesh.cell_nodes, 0].mean(axis=1) > 0.5).astype(np.float64)

    def contrasts(tag, dms, refs, forms):
        right = [right_of(dms[0].mesh)]
        for ref in refs:                                   # the side of a cell crosses a refinement as mu does
            right.append(np.ascontiguousarray(ref.prolong_dg(0, right[-1])).ravel())
        for p in args.degrees:
            hs = []
            for d_ in dms[:-1]:
                bf = d_.mesh.boundary_facets()
                hs.append(cpp.PrimalElasticity(d_, p, 1.0))
                hs[-1].set_dirichlet(bf, bf)
            top, b = make_problem(cpp, torch, dms[-1], p, True)
            hs.append(top)
            mls = {name: cpp.Multilevel(hs, refs, **kw) for name, kw in forms.items()}
            zero = torch.zeros(2 * top.ndofs, dtype=torch.float64, device="cuda")
            for contrast in (1.0, 10.0, 1000.0):
                for h_, rt in zip(hs, right):
                    h_.set_shear(cell_mu=1.0 + (contrast - 1.0) * rt)
                for name, kw in forms.items():
                    if kw.get("coarse"):
                        mls[name].set_coarse(True)         # (the factor is a snapshot of the operator of level 0)
                r = dict(levels=len(dms), cells=dms[-1].mesh.ncells, rows=2 * top.ndofs, contrast=contrast)
                for name, h_ in [("jacobi", top)] + list(mls.items()):
                    info, ms, _ = timed_solve(torch, h_, b, zero, 1e-8, args.maxit)
                    r[name] = dict(iterations=info["iterations"], ms=ms, converged=info["converged"],
                                   breakdown=info["breakdown"])
                say(f"{tag} E_{p} contrast {contrast:g}: " + "; ".join(
                    f"{name} {r[name]['iterations']} iterations in {r[name]['ms']:.1f} ms"
                    for name in ["jacobi"] + list(forms)) + f" ({r['levels']} levels, {r['cells']} cells, one run each)")
                res[f"SHEAR_{tag}_E{p}_contrast{contrast:g}"] = r
            for ml in mls.values():
                ml.close()
            for h_ in hs:
                h_.close()

    dms, refs, _ = device_hierarchy(args, cpp)
    contrasts("UNIFORM", dms, refs, dict(hierarchy=dict()))
    base = create_unit_square(16, shuffle_seed=3)
    dms, refs = [cpp.DeviceMesh(base)], []
    for _ in range(10):
        m = dms[-1].mesh
        on = np.abs(m.x[m.cell_nodes, 0] - 0.5).min(axis=1) < 1e-12
        refs.append(dms[-1].refine(np.nonzero(on)[0].astype(np.int32), keep_plan=True))
        dms.append(refs[-1].dmesh)
    say(f"adaptive hierarchy: cells {[d_.mesh.ncells for d_ in dms]}")
    contrasts("ADAPTIVE", dms, refs, dict(hierarchy=dict(), local_coarse=dict(local=True, coarse=True)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=500, help="squares per side (4 n^2 triangles)")
    ap.add_argument("--degrees", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--products", type=int, default=200)
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--maxit", type=int, default=100000)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--host-budget", type=float, default=150.0, help="seconds for the host cg")
    ap.add_argument("--spsolve-degrees", type=int, nargs="*", default=[1],
                    help="degrees at which --host also runs spsolve (P_2 at 1M triangles takes minutes and many GB)")
    ap.add_argument("--elasticity", action="store_true", help="the same figures for cpp.PrimalElasticity as well")
    ap.add_argument("--multilevel", action="store_true", help="the figures of the multilevel preconditioner instead")
    ap.add_argument("--coarse-n", type=int, default=2, help="--multilevel: squares per side of the coarsest mesh")
    ap.add_argument("--nrhs", type=int, nargs="+", default=[], metavar="R",
                    help="several right-hand sides in one call against one call each, on the hierarchy of --multilevel")
    ap.add_argument("--repeats", type=int, default=5,
                    help="--nrhs, --reaction: timed repeats of every pair (at least 5)")
    ap.add_argument("--reaction", action="store_true", help="the figures of the reaction term instead")
    ap.add_argument("--taus", type=float, nargs="+", default=[1e-2, 1e-4], metavar="TAU",
                    help="--reaction --multilevel: the time steps of the heat step, next to c = 0")
    ap.add_argument("--plain-only", action="store_true",
                    help="--reaction: time the product without the term alone (runs on a library without the term too)")
    ap.add_argument("--shear", action="store_true", help="the figures of the cell-wise shear modulus instead")
    ap.add_argument("--diffusion", action="store_true", help="the figures of the cell-wise diffusion tensor instead")
    ap.add_argument("--check-every", nargs="*", default=[], metavar="LIB:N")
    ap.add_argument("--check-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.products < 100:
        ap.error("--products: at least 100")
    if args.repeats < 5 or any(r < 1 for r in args.nrhs):
        ap.error("--repeats: at least 5; --nrhs: at least 1")
    res = {}
    if not args.check_only:
        for item in args.check_every:
            lib, n = item.rsplit(":", 1)
            env = dict(os.environ, EQLB_AMD_LIB=os.path.abspath(lib))
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--n", str(args.n), "--degrees", "2",
                                  "--check-only", "--maxit", str(args.maxit)], env=env, capture_output=True, text=True,
                                 timeout=600)
            last = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
            if out.returncode != 0 or not last:
                say(f"check-every {n}: child failed ({out.returncode}): {out.stderr[-400:]}")
                sys.exit(1)
            z = json.loads(last[-1])["P2"]
            res.setdefault("check_every", {})[n] = dict(ms=z["zero"]["ms"], iterations=z["zero"]["iterations"],
                                                        iteration_ms=z["iteration_ms"])
            say(f"EQLB_PRIMAL_CHECK_EVERY = {n}: P_2 to rtol 1e-8 from zero {z['zero']['ms']:.1f} ms, "
                f"{z['zero']['iterations']} iterations; iteration {z['iteration_ms']:.4f} ms")
    import torch
    torch.cuda.init()
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.mesh import create_unit_square
    if args.reaction:
        run_reaction(args, cpp, torch, res)
        print(json.dumps(res))
        return
    if args.shear:
        run_shear(args, cpp, torch, res)
        print(json.dumps(res))
        return
    if args.diffusion:
        run_diffusion(args, cpp, torch, res)
        print(json.dumps(res))
        return
    if args.nrhs:
        run_many(args, cpp, torch, res)
        print(json.dumps(res))
        return
    if args.multilevel:
        run_multilevel(args, cpp, torch, res)
        print(json.dumps(res))
        return
    t0 = time.perf_counter()
    dm = cpp.DeviceMesh(create_unit_square(args.n, shuffle_seed=3, perturb=0.15))
    say(f"mesh: {dm.mesh.ncells} cells in {time.perf_counter() - t0:.1f} s")
    for p in args.degrees:
        run_degree(args, cpp, torch, dm, p, res)
    if args.elasticity and not args.check_only:
        for p in args.degrees:
            run_degree(args, cpp, torch, dm, p, res, elasticity=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
