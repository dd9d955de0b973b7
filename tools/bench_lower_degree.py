#!/usr/bin/env python3
"""Time the semi-explicit sweep with projected data of degree k-2 against degree k-1 on the 1M-triangle crossed mesh.

  python tools/bench_lower_degree.py [--n 500] [--ks 2 3] [--steps 20] [--warmup 3] [--windows 5]

Per k three variants, through the C ABI on device memory (torch's current stream), timed with HIP events:
  native    (k, k-2): the data read in DG_{k-2} by the lower-degree kernels
  same      (k, k-1): data of degree k-1 on the same mesh (the headline configuration at k = 2)
  embedded  DG_{k-2} data embedded into DG_{k-1} on the device (torch matmul with the embed_dg matrix), then the
            (k, k-1) step - the route a caller with device-resident DG_{k-2} data had before
All variants run in one process after the warm-up and the clock-settle probes of bench.py (probes of K steps for at
least 40 ms until two agree within 1 %), then in alternating order in `--windows` windows of K steps each.  Prints
one JSON object: ms per step (median and spread over the windows) and the compulsory bytes per cell from the shapes.
The kernel time of the same runs: `rocprofv3 --kernel-trace --stats -- python tools/bench_lower_degree.py ...`.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def bytes_per_cell(k, d, nrhs=1):
    """8 R [2 nd + nd + k(k+2)] + 24: G (2 nd), f (nd), the RT_k result, J (3 doubles) of a cell."""
    nd = (d + 1) * (d + 2) // 2
    return 8 * nrhs * (3 * nd + k * (k + 2)) + 24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--ks", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()

    import torch  # first: its HIP runtime is the one the library binds to (bench.py)
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.elmtlib.lagrange import Lagrange
    from dolfinx_eqlb_amd.mesh import create_unit_square
    from synthetic import facet_types, make_compatible_data

    dev = torch.device("cuda:0")
    torch.cuda.init()
    mesh = create_unit_square(args.n, shuffle_seed=1234)
    ft = facet_types(mesh)
    dm = cpp.DeviceMesh(mesh)
    nc = mesh.ncells
    stream = torch.cuda.current_stream().cuda_stream
    steps = {}
    keep = []
    for k in args.ks:
        lo, hi = k - 2, k - 1
        nrt = k * (k + 2)
        x = torch.zeros(nc * nrt, dtype=torch.float64, device=dev)
        keep.append(x)
        Gl, fl = make_compatible_data(mesh, k, ft, degree_dg=lo)
        Gh, fh = make_compatible_data(mesh, k, ft, degree_dg=hi)
        gl, fl_d = torch.from_numpy(Gl).to(dev), torch.from_numpy(fl).to(dev)
        gh, fh_d = torch.from_numpy(Gh).to(dev), torch.from_numpy(fh).to(dev)
        ndl, ndh = Lagrange(lo).ndofs, Lagrange(hi).ndofs
        nodes = np.array([[float(a), float(b)] for a, b in Lagrange(hi).nodes])
        E = torch.from_numpy(np.ascontiguousarray(Lagrange(lo).tabulate(nodes)[0])).to(dev)  # [nd_hi, nd_lo]
        ge = torch.empty(nc * ndh * 2, dtype=torch.float64, device=dev)
        fe = torch.empty(nc * ndh, dtype=torch.float64, device=dev)
        keep += [gl, fl_d, gh, fh_d, E, ge, fe]
        eq_lo = cpp.SemiExplicitEquilibrator(dm, k, 1, degree_dg=lo)
        eq_hi = cpp.SemiExplicitEquilibrator(dm, k, 1)
        for eq in (eq_lo, eq_hi):
            eq.set_option("accumulate", 0)
            eq.set_boundary(ft)
        keep += [eq_lo, eq_hi]

        def native(eq=eq_lo, g=gl, f=fl_d, x=x):
            eq.equilibrate_device(g.data_ptr(), f.data_ptr(), x.data_ptr(), stream)

        def same(eq=eq_hi, g=gh, f=fh_d, x=x):
            eq.equilibrate_device(g.data_ptr(), f.data_ptr(), x.data_ptr(), stream)

        def embedded(eq=eq_hi, g=gl, f=fl_d, E=E, ge=ge, fe=fe, x=x, ndl=ndl, ndh=ndh):
            torch.matmul(E, g.view(nc, ndl, 2), out=ge.view(nc, ndh, 2))
            torch.matmul(f.view(nc, ndl), E.t(), out=fe.view(nc, ndh))
            eq.equilibrate_device(ge.data_ptr(), fe.data_ptr(), x.data_ptr(), stream)

        steps[f"k{k}_native_d{lo}"] = (native, bytes_per_cell(k, lo))
        steps[f"k{k}_same_mesh_d{hi}"] = (same, bytes_per_cell(k, hi))
        steps[f"k{k}_embedded_d{lo}_to_d{hi}"] = (embedded, bytes_per_cell(k, hi) + 8 * 3 * (ndl + ndh))
    for name, (fn, _) in steps.items():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    for eq in [o for o in keep if isinstance(o, cpp.SemiExplicitEquilibrator)]:
        eq.check_status(stream)
    # clock settle (as bench.py): probes of K steps of every variant, at least 40 ms, until two agree within 1 %
    settle, t0 = [], time.perf_counter()
    while len(settle) < 24:
        tp = time.perf_counter()
        for fn, _ in steps.values():
            for _ in range(args.steps):
                fn()
        torch.cuda.synchronize()
        settle.append(time.perf_counter() - tp)
        if len(settle) >= 2 and (time.perf_counter() - t0) >= 0.04 and abs(settle[-1] - settle[-2]) <= 0.01 * settle[-2]:
            break
    ms = {name: [] for name in steps}
    names = list(steps)
    for w in range(args.windows):
        order = names if w % 2 == 0 else names[::-1]  # alternate the order of the variants between windows
        for name in order:
            fn = steps[name][0]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.steps)
    out = {"mesh": f"crossed {args.n}x{args.n}", "ncells": nc, "steps": args.steps, "windows": args.windows,
           "settle_probes": len(settle), "variants": {}}
    for name, v in ms.items():
        bpc = steps[name][1]
        med = float(np.median(v))
        out["variants"][name] = {"ms_per_step": med, "min": float(np.min(v)), "max": float(np.max(v)),
                                 "spread": float((np.max(v) - np.min(v)) / med), "bytes_per_cell": bpc,
                                 "effective_TBps": bpc * nc / (med * 1e-3) / 1e12}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
