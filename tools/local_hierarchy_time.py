#!/usr/bin/env python3
"""local_hierarchy_time.py: local smoothing against the full multilevel sum on a graded hierarchy at about 1M triangles.

The hierarchy is refined on the device: from create_unit_square(--coarse-n), every step marks the --frac of the cells
whose centroid is nearest the corner (0, 0) (stable argsort of the distance, on the exported mesh) and refines them with
the plan kept (DeviceMesh.refine(..., keep_plan=True)), until the next step would pass --cells.  One solver handle per
level, Dirichlet all around, coefficients 1.  The right-hand side (--rhs): "load", that of tools/primal_solve_time.py
(the smooth f_ex projected to DG_{p-1}; for elasticity the body force (f_ex, f_ex(y, x))), or "random", standard normal
(seed 1) on the free rows - every frequency at once, the right-hand side of the CPU figures of the numpy statement.

For every degree of --degrees, for Poisson and (with --elasticity) for elasticity, on the SAME handles and the same
cpp.Multilevel in one process, with the switch off ("full") and on ("local"):
  levels, rows over all levels, active rows (sum of active_count over the levels)
  iterations to rtol 1e-8 from zero
  time per solve: wall time of solve_raw, which waits for the device; median and spread (max - min) of --repeats (>= 5)
             after clock-settle probes (repeated for at least 40 ms and until two agree within 1 %, at most 24)
  time per application: device events around --products (>= 100) calls of precondition_raw after a warm-up, repeated
             --repeats times: median and spread
and the Jacobi entry of the finest handle (iterations, one timed solve) for scale.  Per application the two rules do the
same launches and nearly the same traffic; the gain, if any, is the iteration ratio.
Prints one line per figure, a table, and last one JSON line with all of them.  Nothing here is a pass/fail condition.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from primal_solve_time import make_problem, say, settle_probes, timed_calls  # noqa: E402


def corner_marks(mesh, frac):
    xc = mesh.x[mesh.cell_nodes, :2].mean(axis=1)
    order = np.argsort(np.linalg.norm(xc, axis=1), kind="stable")
    return np.sort(order[:max(1, int(frac * mesh.ncells))]).astype(np.int32)


def graded_hierarchy(args, cpp):
    """(DeviceMesh per level, Refinement per link, cells per level)"""
    from dolfinx_eqlb_amd.mesh import create_unit_square
    t0 = time.perf_counter()
    dms, refs = [cpp.DeviceMesh(create_unit_square(args.coarse_n))], []
    while True:
        ref = dms[-1].refine(corner_marks(dms[-1].mesh, args.frac), keep_plan=True)
        if ref.dmesh.mesh.ncells > args.cells and refs:
            ref.close()
            break
        refs.append(ref)
        dms.append(ref.dmesh)
    cells = [d.mesh.ncells for d in dms]
    say(f"hierarchy: {len(dms)} levels, cells {cells} in {time.perf_counter() - t0:.1f} s")
    return dms, refs, cells


def timed_solves(torch, h, b, n, maxit, repeats):
    """(info, wall ms of every repeat, probes) of solve_raw to rtol 1e-8 from zero"""
    u = torch.zeros(n, dtype=torch.float64, device="cuda")
    info = [None]

    def solve():
        u.zero_()
        torch.cuda.synchronize()
        info[0] = h.solve_raw(b.data_ptr(), u.data_ptr(), 1e-8, 0.0, maxit)

    probes = settle_probes(solve)
    times = []
    for _ in range(repeats):
        u.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info[0] = h.solve_raw(b.data_ptr(), u.data_ptr(), 1e-8, 0.0, maxit)
        times.append((time.perf_counter() - t0) * 1e3)
    return info[0], times, len(probes)


def run(args, cpp, torch, dms, refs, cells, p, elasticity, res):
    bs, P = (2, "E") if elasticity else (1, "P")
    hs = []
    for dm in dms[:-1]:
        bf = dm.mesh.boundary_facets()
        hs.append(cpp.PrimalElasticity(dm, p, 1.0) if elasticity else cpp.PrimalPoisson(dm, p))
        hs[-1].set_dirichlet(*([bf, bf] if elasticity else [bf]))
    top, b = make_problem(cpp, torch, dms[-1], p, elasticity)
    hs.append(top)
    ml = cpp.Multilevel(hs, refs)
    n = bs * top.ndofs
    if args.rhs == "random":
        from dolfinx_eqlb_amd.lsolver import primal
        mesh = dms[-1].mesh
        fixed = np.repeat(primal.dirichlet_mask(mesh, p, mesh.boundary_facets()), bs)
        b = torch.from_numpy(np.where(fixed, 0.0, np.random.default_rng(1).standard_normal(n))).cuda()
    rows = sum(ml.nrows)
    r = dict(levels=len(dms), cells=cells[-1], fine_rows=n, rows_all_levels=rows, repeats=args.repeats, rhs=args.rhs)
    x = torch.from_numpy(np.random.default_rng(0).standard_normal(n)).cuda()
    z = torch.empty_like(x)
    for name, on in (("full", False), ("local", True)):
        ml.local = on
        active = sum(ml.active_count(l) for l in range(ml.nlevels)) if on else rows
        info, times, probes = timed_solves(torch, ml, b, n, args.maxit, args.repeats)
        app = [timed_calls(torch, lambda: ml.precondition_raw(x.data_ptr(), z.data_ptr()), args.products)
               for _ in range(args.repeats)]
        r[name] = dict(active_rows=active, iterations=info["iterations"], converged=info["converged"],
                       replacements=info["replacements"], breakdown=info["breakdown"], settle_probes=probes,
                       solve_ms=dict(median=float(np.median(times)), spread=float(np.ptp(times)), all=times),
                       application_ms=dict(median=float(np.median(app)), spread=float(np.ptp(app)), all=app))
        say(f"{P}_{p} {name}: {r['levels']} levels, {rows} rows over all levels, {active} active; "
            f"{info['iterations']} iterations (converged {info['converged']}); solve {r[name]['solve_ms']['median']:.2f} ms "
            f"(spread {r[name]['solve_ms']['spread']:.2f}) over {args.repeats} repeats after {probes} probes; application "
            f"{r[name]['application_ms']['median']:.4f} ms (spread {r[name]['application_ms']['spread']:.4f})")
    ml.local = False
    info, times, _ = timed_solves(torch, top, b, n, args.maxit, 1)
    r["jacobi"] = dict(iterations=info["iterations"], converged=info["converged"], solve_ms=times[0])
    say(f"{P}_{p} jacobi: {info['iterations']} iterations (converged {info['converged']}), solve {times[0]:.2f} ms")
    r["iteration_ratio"] = r["local"]["iterations"] / max(r["full"]["iterations"], 1)
    r["solve_ratio"] = r["local"]["solve_ms"]["median"] / r["full"]["solve_ms"]["median"]
    ml.close()
    res[f"{P}{p}"] = r


def table(res):
    say("| problem | levels | cells | fine rows | rows over all levels | active rows | full BPX: iterations, ms (spread) | "
        "local: iterations, ms (spread) | application full / local, ms | Jacobi: iterations, ms |")
    say("|---|---|---|---|---|---|---|---|---|---|")
    for key, r in res.items():
        f, lo, j = r["full"], r["local"], r["jacobi"]
        say(f"| {key} | {r['levels']} | {r['cells']} | {r['fine_rows']} | {r['rows_all_levels']} | {lo['active_rows']} | "
            f"{f['iterations']}, {f['solve_ms']['median']:.1f} ({f['solve_ms']['spread']:.1f}) | "
            f"{lo['iterations']}, {lo['solve_ms']['median']:.1f} ({lo['solve_ms']['spread']:.1f}) | "
            f"{f['application_ms']['median']:.3f} / {lo['application_ms']['median']:.3f} | "
            f"{j['iterations']}, {j['solve_ms']:.1f} |")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--coarse-n", type=int, default=16, help="squares per side of the coarsest mesh (4 n^2 triangles)")
    ap.add_argument("--frac", type=float, default=0.15, help="share of the cells marked per step")
    ap.add_argument("--cells", type=int, default=1_000_000, help="the finest level has at most this many cells")
    ap.add_argument("--degrees", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--elasticity", action="store_true", help="the elasticity solve as well")
    ap.add_argument("--rhs", choices=("load", "random"), default="load", help="the right-hand side of the solves")
    ap.add_argument("--products", type=int, default=100, help="applications per timed batch (at least 100)")
    ap.add_argument("--repeats", type=int, default=5, help="timed repeats (at least 5)")
    ap.add_argument("--maxit", type=int, default=100000)
    args = ap.parse_args()
    if args.products < 100 or args.repeats < 5:
        ap.error("--products: at least 100; --repeats: at least 5")
    if not 0.0 < args.frac <= 1.0:
        ap.error("--frac: in (0, 1]")
    import torch
    torch.cuda.init()
    from dolfinx_eqlb_amd import cpp
    dms, refs, cells = graded_hierarchy(args, cpp)
    res = {}
    for elasticity in ([False, True] if args.elasticity else [False]):
        for p in args.degrees:
            run(args, cpp, torch, dms, refs, cells, p, elasticity, res)
    table(res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
