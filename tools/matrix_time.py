#!/usr/bin/env python3
"""matrix_time.py: timings of the assembled P_p operators (cpp.PrimalPoisson.matrix, cpp.PrimalElasticity.matrix,
cpp.csr_apply) at about 1M triangles, against the matrix-free product of the same handle in the same process.

On create_unit_square(N, shuffle_seed=3, perturb=0.15) (N = 500: 1,000,000 cells), for P_1 and P_2 Poisson (kappa = 1)
and [P_1]^2 and [P_2]^2 elasticity (pi_1 = 1), Dirichlet all around:
  pattern    wall time of eqlb_*_matrix_pattern (it waits for the count by nature) after eqlb_*_matrix_release, --repeats
             times; nnz, and the work space: the two key arrays and the kept arrays from the shapes (the library prints
             its own figure with the temporary storage of the sort on stderr: EQLB_PROFILE_SETUP is set here)
  fill       device time of one eqlb_*_matrix_values (raw) into device memory
  product    device time of one eqlb_csr_apply against one matrix-free apply (masked = 0) ON THE SAME HANDLE, in
             alternating blocks; the bytes either reads and writes, from the shapes, and the achieved bytes/s
Every device time is the median of --repeats (>= 5) blocks of --calls calls by device events, after clock-settle probes
as bench.py runs them (repeated for at least 40 ms and until two agree within 1 %, at most 24); the spread (max - min)
stands beside it.  --apply-only: the matrix-free product alone - runs on a library without the matrix entries too
(EQLB_AMD_LIB), for the A/B against the parent commit (tools/build_head.sh) in one session.  --product-only: one
pattern build and the two products, for builds with other values of EQLB_CSR_GROUP and EQLB_CSR_GROUP_MIN
(tools/build_variant.sh NAME "-D..." eqlb_primal_matrix, EQLB_AMD_LIB).
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


def blocks(torch, args, fns, probe):
    """{name: dict(median_ms, spread_ms, all_ms)} of the calls fns = {name: call}, in alternating blocks"""
    probes = settle_probes(probe)
    t = {k: [] for k in fns}
    for _ in range(args.repeats):
        for k, call in fns.items():
            t[k].append(timed_calls(torch, call, args.calls))
    r = {k: dict(median_ms=float(np.median(v)), spread_ms=float(np.ptp(v)), all_ms=v) for k, v in t.items()}
    r["settle_probes"] = len(probes)
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--degrees", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--apply-only", action="store_true")
    ap.add_argument("--product-only", action="store_true", help="one pattern build, no fill blocks: the two products")
    args = ap.parse_args()
    if args.repeats < 5 or args.calls < 1:
        ap.error("--repeats at least 5, --calls at least 1")
    os.environ.setdefault("EQLB_PROFILE_SETUP", "1")
    import torch
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.mesh import create_unit_square
    if not torch.cuda.is_available() or cpp.device_count() < 1:
        say("matrix_time.py: no device")
        sys.exit(1)
    t0 = time.perf_counter()
    dm = cpp.DeviceMesh(create_unit_square(args.n, shuffle_seed=3, perturb=0.15))
    nc = dm.mesh.ncells
    say(f"{nc} cells ({time.perf_counter() - t0:.1f} s); library {cpp.LIB_PATH}")
    res = dict(cells=nc, calls=args.calls, repeats=args.repeats, library=cpp.LIB_PATH)
    bf = dm.mesh.boundary_facets()
    for problem in ("poisson", "elasticity"):
        for p in args.degrees:
            bs = 1 if problem == "poisson" else 2
            tag = f"P{p}" if bs == 1 else f"E{p}"
            h = cpp.PrimalPoisson(dm, p) if bs == 1 else cpp.PrimalElasticity(dm, p, 1.0)
            h.set_dirichlet(*([bf] * bs))
            n = bs * h.ndofs
            nd = (p + 1) * (p + 2) // 2
            x = torch.from_numpy(np.random.default_rng(0).standard_normal(n)).cuda()
            y = torch.empty_like(x)

            def free():
                h.apply_raw(x.data_ptr(), y.data_ptr(), False)

            def probe():
                free()
                torch.cuda.synchronize()

            # the store-and-sum product: dofmap, J, y_loc written and read, slots, x gathered, y
            free_bytes = nc * nd * 4 + nc * 32 + 2 * bs * nc * nd * 8 + 3 * nc * p * 4 + bs * nc * nd * 8 + n * 8
            r = dict(rows=n)
            if args.apply_only:
                b = blocks(torch, args, {"free": free}, probe)
                r.update(free=b["free"], settle_probes=b["settle_probes"], free_bytes=free_bytes)
                say(f"{tag}: {n} rows; matrix-free product {b['free']['median_ms']:.4f} ms (spread "
                    f"{b['free']['spread_ms']:.4f}); median of {args.repeats} blocks of {args.calls} calls after "
                    f"{b['settle_probes']} probes")
                res[tag] = r
                h.close()
                continue
            tp = []
            for _ in range(1 if args.product_only else args.repeats):
                h.matrix_release()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                nnz = h.matrix_pattern_raw()
                tp.append((time.perf_counter() - t1) * 1e3)
            keys = 2 * 8 * nc * nd * nd
            kept = 8 * (h.ndofs + 1) + 8 * (nnz // (bs * bs))
            r.update(nnz=nnz, pattern=dict(median_ms=float(np.median(tp)), spread_ms=float(np.ptp(tp)), all_ms=tp),
                     key_bytes=keys, kept_bytes=kept)
            say(f"{tag}: {n} rows, nnz {nnz} ({nnz / n:.1f} per row); pattern build {np.median(tp):.2f} ms (spread "
                f"{np.ptp(tp):.2f}, {args.repeats} builds); work space: keys {keys / 1e6:.0f} MB + the sort's temporary "
                f"storage (stderr), kept {kept / 1e6:.0f} MB")
            ip = torch.empty(n + 1, dtype=torch.int64, device="cuda")
            ix = torch.empty(nnz, dtype=torch.int32, device="cuda")
            v = torch.empty(nnz, dtype=torch.float64, device="cuda")
            h.matrix_export_raw(ip.data_ptr(), ix.data_ptr())
            h.matrix_values_raw(0, v.data_ptr(), nnz)
            torch.cuda.synchronize()
            z = torch.empty_like(x)

            def fill():
                h.matrix_values_raw(0, v.data_ptr(), nnz)

            def csr():
                cpp.csr_apply_raw(n, ip.data_ptr(), ix.data_ptr(), v.data_ptr(), x.data_ptr(), z.data_ptr())

            if not args.product_only:
                b = blocks(torch, args, {"fill": fill}, probe)
                r["fill"] = b["fill"]
                say(f"{tag}: fill {b['fill']['median_ms']:.4f} ms (spread {b['fill']['spread_ms']:.4f})")
            b = blocks(torch, args, {"free": free, "csr": csr}, probe)
            csr_bytes = nnz * 12 + (n + 1) * 8 + 2 * n * 8
            r.update(free=b["free"], csr=b["csr"], settle_probes=b["settle_probes"], free_bytes=free_bytes,
                     csr_bytes=csr_bytes, ratio=b["csr"]["median_ms"] / b["free"]["median_ms"])
            diff = abs(b["csr"]["median_ms"] - b["free"]["median_ms"])
            r["difference_exceeds_spread"] = bool(diff > max(b["csr"]["spread_ms"], b["free"]["spread_ms"]))
            free()
            csr()
            torch.cuda.synchronize()
            r["max_abs_difference"] = float((y - z).abs().max())
            say(f"{tag}: product: matrix-free {b['free']['median_ms']:.4f} ms (spread {b['free']['spread_ms']:.4f}, "
                f"{free_bytes / 1e6:.0f} MB, {free_bytes / b['free']['median_ms'] / 1e9:.2f} TB/s), assembled "
                f"{b['csr']['median_ms']:.4f} ms (spread {b['csr']['spread_ms']:.4f}, {csr_bytes / 1e6:.0f} MB, "
                f"{csr_bytes / b['csr']['median_ms'] / 1e9:.2f} TB/s) = {r['ratio']:.3f} of it; the difference exceeds "
                f"the spread: {r['difference_exceeds_spread']}; max |difference| of the results "
                f"{r['max_abs_difference']:.2e}; median of {args.repeats} blocks of {args.calls} calls after "
                f"{b['settle_probes']} probes")
            res[tag] = r
            h.close()
            del ip, ix, v
    say(json.dumps(res))


if __name__ == "__main__":
    main()
