#!/usr/bin/env python3
"""coarse_solve_time.py: the exact solve on level 0 of the multilevel preconditioner (cpp.Multilevel(..., coarse=True))
against the diagonal of level 0, under the full sum and under local smoothing, on a graded hierarchy at about 1M
triangles.

The hierarchy is that of tools/local_hierarchy_time.py (from create_unit_square(--coarse-n), every step refines the
--frac of the cells nearest the corner (0, 0) on the device with the plan kept, until the next step would pass --cells);
one solver handle per level, Dirichlet all around, coefficients 1, the right-hand side --rhs of that tool.

For every degree of --degrees, for Poisson and (with --elasticity) for elasticity, on the SAME handles and the same
cpp.Multilevel in one process, for full / local x coarse off / on:
  iterations to rtol 1e-8 from zero
  time per solve: wall time of solve_raw, which waits for the device
  time per application: device events around --products (>= 100) calls of precondition_raw after a warm-up
and the set-up time of set_coarse(True) (wall time: it waits for the device; every call factors again) with the number
of coarse rows.  Each time is the median and the spread (max - min) of --repeats (>= 5) runs after clock-settle probes
(repeated for at least 40 ms and until two agree within 1 %, at most 24).

--setup-sizes instead: one-level hierarchies with about 500, 2 000 and 4 000 free rows (create_unit_square(8) and (16) at
P_2, create_unit_square(45) at P_1): the set-up time of set_coarse and the time of one application of the factor.

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

from local_hierarchy_time import graded_hierarchy, timed_solves  # noqa: E402
from primal_solve_time import make_problem, say, settle_probes, timed_calls  # noqa: E402

COMBINATIONS = (("full", False, False), ("local", True, False), ("full+coarse", False, True),
                ("local+coarse", True, True))


def stats(times):
    return dict(median=float(np.median(times)), spread=float(np.ptp(times)), all=[float(t) for t in times])


def timed_setup(ml, repeats):
    """(wall ms of every repeat of set_coarse(True), probes)"""
    probes = settle_probes(lambda: ml.set_coarse(True))
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        ml.set_coarse(True)
        times.append((time.perf_counter() - t0) * 1e3)
    return times, len(probes)


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
    r = dict(levels=len(dms), cells=cells[-1], fine_rows=n, repeats=args.repeats, rhs=args.rhs)
    setup, probes = timed_setup(ml, args.repeats)
    r["coarse_rows"] = ml.coarse_rows
    r["setup_ms"] = dict(stats(setup), settle_probes=probes)
    say(f"{P}_{p} set_coarse: {r['coarse_rows']} coarse rows, {r['setup_ms']['median']:.2f} ms "
        f"(spread {r['setup_ms']['spread']:.2f}) over {args.repeats} repeats after {probes} probes")
    x = torch.from_numpy(np.random.default_rng(0).standard_normal(n)).cuda()
    z = torch.empty_like(x)
    for name, local, coarse in COMBINATIONS:
        ml.local = local
        ml.coarse = coarse
        info, times, probes = timed_solves(torch, ml, b, n, args.maxit, args.repeats)
        app = [timed_calls(torch, lambda: ml.precondition_raw(x.data_ptr(), z.data_ptr()), args.products)
               for _ in range(args.repeats)]
        r[name] = dict(iterations=info["iterations"], converged=info["converged"], replacements=info["replacements"],
                       breakdown=info["breakdown"], settle_probes=probes, solve_ms=stats(times), application_ms=stats(app))
        say(f"{P}_{p} {name}: {info['iterations']} iterations (converged {info['converged']}); solve "
            f"{r[name]['solve_ms']['median']:.2f} ms (spread {r[name]['solve_ms']['spread']:.2f}) over {args.repeats} "
            f"repeats after {probes} probes; application {r[name]['application_ms']['median']:.4f} ms "
            f"(spread {r[name]['application_ms']['spread']:.4f})")
    ml.close()
    res[f"{P}{p}"] = r


def table(res):
    say("| problem | levels | cells | fine rows | coarse rows | set_coarse, ms (spread) | "
        + " | ".join(f"{name}: iterations, solve ms (spread), application ms" for name, _, _ in COMBINATIONS) + " |")
    say("|---|---|---|---|---|---|" + "---|" * len(COMBINATIONS))
    for key, r in res.items():
        cols = [f"{r[name]['iterations']}, {r[name]['solve_ms']['median']:.1f} ({r[name]['solve_ms']['spread']:.1f}), "
                f"{r[name]['application_ms']['median']:.3f}" for name, _, _ in COMBINATIONS]
        say(f"| {key} | {r['levels']} | {r['cells']} | {r['fine_rows']} | {r['coarse_rows']} | "
            f"{r['setup_ms']['median']:.1f} ({r['setup_ms']['spread']:.1f}) | " + " | ".join(cols) + " |")


def setup_sizes(args, cpp, torch, res):
    from dolfinx_eqlb_amd.mesh import create_unit_square
    say("| mesh | p | coarse rows | set_coarse, ms (spread) | application of the factor, ms (spread) | Jacobi application, ms |")
    say("|---|---|---|---|---|---|")
    for nsq, p in ((8, 2), (16, 2), (45, 1)):
        dm = cpp.DeviceMesh(create_unit_square(nsq))
        h = cpp.PrimalPoisson(dm, p)
        h.set_dirichlet(dm.mesh.boundary_facets())
        ml = cpp.Multilevel([h], [])
        x = torch.from_numpy(np.random.default_rng(0).standard_normal(h.ndofs)).cuda()
        z = torch.empty_like(x)
        apply = lambda: ml.precondition_raw(x.data_ptr(), z.data_ptr())   # noqa: E731
        jac = stats([timed_calls(torch, apply, args.products) for _ in range(args.repeats)])
        setup, probes = timed_setup(ml, args.repeats)
        app = stats([timed_calls(torch, apply, args.products) for _ in range(args.repeats)])
        r = dict(coarse_rows=ml.coarse_rows, setup_ms=dict(stats(setup), settle_probes=probes), application_ms=app,
                 jacobi_application_ms=jac)
        say(f"| create_unit_square({nsq}) | {p} | {r['coarse_rows']} | {r['setup_ms']['median']:.2f} "
            f"({r['setup_ms']['spread']:.2f}) | {app['median']:.4f} ({app['spread']:.4f}) | {jac['median']:.4f} |")
        res[f"setup{nsq}p{p}"] = r
        ml.close()


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
    ap.add_argument("--setup-sizes", action="store_true",
                    help="instead: set_coarse and one application on one level of about 500, 2 000 and 4 000 free rows")
    args = ap.parse_args()
    if args.products < 100 or args.repeats < 5:
        ap.error("--products: at least 100; --repeats: at least 5")
    if not 0.0 < args.frac <= 1.0:
        ap.error("--frac: in (0, 1]")
    import torch
    torch.cuda.init()
    from dolfinx_eqlb_amd import cpp
    res = {}
    if args.setup_sizes:
        setup_sizes(args, cpp, torch, res)
    else:
        dms, refs, cells = graded_hierarchy(args, cpp)
        for elasticity in ([False, True] if args.elasticity else [False]):
            for p in args.degrees:
                run(args, cpp, torch, dms, refs, cells, p, elasticity, res)
        table(res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
