#!/usr/bin/env python3
"""spring_time.py: what the spring term of cpp.PrimalElasticity (set_springs) costs at about 1M triangles.

On create_unit_square(N, shuffle_seed=3, perturb=0.15) (N = 500: 1,000,000 cells), [P_1]^2 and [P_2]^2 elasticity
(pi_1 = 1), Dirichlet on the side x = 0 in both rows:
  product      device time of one matrix-free apply (masked = 1) with full-rank springs on all four sides against the same
               call without them ON THE SAME HANDLE, in alternating blocks (set_springs between the blocks, outside the
               timing)
  iteration    device time of one PCG iteration: a Jacobi solve of --iterations iterations that cannot converge
               (rtol = 0), divided by their number, with the term and without it as above
  set_springs  wall time of one set_springs of the four sides (host list; it waits for the device by nature)
  flux         device time of one spring_flux (device memory) at 4 points, and of the two update_flux_bc (one per stress
               row) of an RT_2 stress equilibrator that take its output, per step
The term touches O(sqrt N) rows; a difference between the two products above the spread needs an explanation.
Every device time is the median of --repeats (>= 5) blocks of --calls calls by device events, after clock-settle probes
(tools/primal_solve_time.py: settle_probes), the protocol of tools/robin_time.py; the spread (max - min) stands beside
it.  The product without the term against the parent commit's library: this tool with --off-only and EQLB_AMD_LIB
(tools/build_head.sh) in the same session.
Prints one line per figure and, last, one JSON line with all of them.  Nothing here is a pass/fail condition.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from primal_solve_time import settle_probes, timed_calls  # noqa: E402


def say(s):
    print(s, flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--degrees", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--off-only", action="store_true",
                    help="time the product without the term only: runs on a library from before the term existed")
    args = ap.parse_args()
    if args.repeats < 5 or args.calls < 1:
        ap.error("--repeats at least 5, --calls at least 1")
    import torch
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.mesh import create_unit_square
    if not torch.cuda.is_available() or cpp.device_count() < 1:
        say("spring_time.py: no device")
        sys.exit(1)
    t0 = time.perf_counter()
    dm = cpp.DeviceMesh(create_unit_square(args.n, shuffle_seed=3, perturb=0.15))
    mesh = dm.mesh
    nc = mesh.ncells
    say(f"{nc} cells ({time.perf_counter() - t0:.1f} s); library {cpp.LIB_PATH}")
    bf = mesh.boundary_facets().astype(np.int32)
    left = bf[np.abs(mesh.facet_midpoints()[bf][:, 0]) < 1e-9]
    K = np.tile(np.array([10.0, 0.5, 1.0]), (bf.size, 1))
    res = dict(cells=nc, calls=args.calls, repeats=args.repeats, spring_facets=int(bf.size), library=cpp.LIB_PATH)

    def med(v):
        return dict(median_ms=float(np.median(v)), spread_ms=float(np.ptp(v)), all_ms=[float(t) for t in v])

    for p in args.degrees:
        h = cpp.PrimalElasticity(dm, p)
        h.set_dirichlet(left, left)
        n = 2 * h.ndofs
        x = torch.from_numpy(np.random.default_rng(0).standard_normal(n)).cuda()
        y = torch.empty_like(x)
        b = torch.from_numpy(np.random.default_rng(1).standard_normal(n)).cuda()
        u = torch.zeros_like(x)

        def product():
            h.apply_raw(x.data_ptr(), y.data_ptr(), True)

        def iterations():
            u.zero_()
            h.solve_raw(b.data_ptr(), u.data_ptr(), 0.0, 0.0, args.iterations)

        def probe():
            product()
            torch.cuda.synchronize()

        probes = settle_probes(probe)
        if args.off_only:
            off = med([timed_calls(torch, product, args.calls) for _ in range(args.repeats)])
            say(f"P{p}: product without the term {off['median_ms']:.4f} ms (spread {off['spread_ms']:.4f}); {n} rows; "
                f"median of {args.repeats} blocks of {args.calls} calls after {len(probes)} probes")
            res[f"P{p}"] = dict(rows=n, product=dict(off=off))
            h.close()
            continue
        t = {(w, s): [] for w in ("product", "iteration") for s in ("on", "off")}
        tset = []
        for _ in range(args.repeats):
            for state in ("on", "off"):
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                if state == "on":
                    h.set_springs(bf, facet_k=K)
                    tset.append((time.perf_counter() - t1) * 1e3)
                else:
                    h.set_springs([])
                t["product", state].append(timed_calls(torch, product, args.calls))
                t["iteration", state].append(timed_calls(torch, iterations, max(1, args.calls // 20)) / args.iterations)
        r = dict(rows=n, settle_probes=len(probes), set_springs=med(tset))
        for what in ("product", "iteration"):
            on, off = med(t[what, "on"]), med(t[what, "off"])
            diff = on["median_ms"] - off["median_ms"]
            r[what] = dict(on=on, off=off, difference_ms=diff,
                           difference_exceeds_spread=bool(abs(diff) > max(on["spread_ms"], off["spread_ms"])))
            say(f"P{p}: {what}: with the term {on['median_ms']:.4f} ms (spread {on['spread_ms']:.4f}), without "
                f"{off['median_ms']:.4f} ms (spread {off['spread_ms']:.4f}): difference {diff:+.4f} ms, exceeds the spread: "
                f"{r[what]['difference_exceeds_spread']}")
        say(f"P{p}: set_springs of {bf.size} facets: {r['set_springs']['median_ms']:.2f} ms wall (spread "
            f"{r['set_springs']['spread_ms']:.2f}); {n} rows; median of {args.repeats} blocks of {args.calls} calls after "
            f"{len(probes)} probes")
        # the flux conditions per step: spring_flux into device memory, then update_flux_bc on both stress rows
        h.set_springs(bf, facet_k=K)
        k = 2
        s, wq = np.array([0.0694318442029737, 0.3300094782075719, 0.6699905217924281, 0.9305681557970263]), \
            np.array([0.1739274225687269, 0.3260725774312731, 0.3260725774312731, 0.1739274225687269])
        g = torch.empty(2 * bf.size * s.size, dtype=torch.float64, device="cuda")
        row = bf.size * s.size * 8
        d_f = torch.from_numpy(bf).cuda()
        ft = np.zeros((2, mesh.nfacets), dtype=np.int8)
        ft[:, bf] = 2
        eq = cpp.SemiExplicitEquilibrator(dm, k, 2, reconstruct_stress=True)
        eq.set_boundary(ft)

        def flux():
            h.spring_flux_raw(x.data_ptr(), s, None, g.data_ptr())

        def update():
            for rr in range(2):
                eq.update_flux_bc_raw(rr, bf.size, d_f.data_ptr(), g.data_ptr() + rr * row, s, wq, False)

        flux()
        update()     # (the first update allocates the table)
        torch.cuda.synchronize()
        tf = [timed_calls(torch, flux, args.calls) for _ in range(args.repeats)]
        tu = [timed_calls(torch, update, args.calls) for _ in range(args.repeats)]
        r["spring_flux"], r["update_flux_bc"] = med(tf), med(tu)
        say(f"P{p}: spring_flux at {s.size} points of {bf.size} facets {r['spring_flux']['median_ms']:.4f} ms (spread "
            f"{r['spring_flux']['spread_ms']:.4f}); update_flux_bc on both rows (RT_2) "
            f"{r['update_flux_bc']['median_ms']:.4f} ms (spread {r['update_flux_bc']['spread_ms']:.4f})")
        res[f"P{p}"] = r
        del eq
        h.close()
    say(json.dumps(res))


if __name__ == "__main__":
    main()
