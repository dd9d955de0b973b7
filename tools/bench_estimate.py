#!/usr/bin/env python3
"""Time eqlb_se_estimate_dg with device-resident DG_d data on the 1M-triangle crossed mesh.

  python tools/bench_estimate.py [--n 500] [--pairs 2,1 2,0 3,2 3,1 3,0] [--steps 20] [--warmup 3] [--windows 5]

Per pair (k, d) the call with all three outputs (cell_div2, cell_sig2, facet_jump) through the C ABI on device
memory (torch's current stream), timed with HIP events.  A call includes what the entry point does around its two
kernels: the upload of the reference tensors and the synchronisation before they are freed.  Next to every d < k-1
figure: what the same result costs without the _dg entry point - lsolver.embed_dg of flux_dg and rhs_dg on the host
(numpy, wall time; the transfers to and from the host that a caller with device-resident data needs on top are not
counted) and the DG_{k-1} call on the embedded data.
All variants run in one process after the warm-up and the clock-settle probes of bench.py (probes of K steps for at
least 40 ms until two agree within 1 %), then in alternating order in `--windows` windows of K steps each.  Prints
one JSON object: ms per call (median and spread over the windows) and the bytes of flux_dg + rhs_dg read per cell,
24 nd(d) (3 nd(d) doubles).
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


def nd_of(d):
    return (d + 1) * (d + 2) // 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--pairs", nargs="+", default=["2,1", "2,0", "3,2", "3,1", "3,0"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    pairs = [tuple(int(v) for v in p.split(",")) for p in args.pairs]

    import torch  # first: its HIP runtime is the one the library binds to (bench.py)
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.lsolver import embed_dg
    from dolfinx_eqlb_amd.mesh import create_unit_square

    dev = torch.device("cuda:0")
    torch.cuda.init()
    mesh = create_unit_square(args.n, shuffle_seed=1234)
    dm = cpp.DeviceMesh(mesh)
    nc = mesh.ncells
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(0)
    outs = [torch.empty(n, dtype=torch.float64, device=dev) for n in (nc, nc, mesh.nfacets)]
    steps, host_ms, keep = {}, {}, []
    for k, d in pairs:
        x = torch.from_numpy(rng.standard_normal(nc * k * (k + 2))).to(dev)
        G, f = rng.standard_normal(nc * nd_of(d) * 2), rng.standard_normal(nc * nd_of(d))
        g_d, f_d = torch.from_numpy(G).to(dev), torch.from_numpy(f).to(dev)
        keep += [x, g_d, f_d]

        def native(k=k, d=d, x=x, g=g_d, f=f_d):
            cpp.estimate_raw(dm, k, 1, x.data_ptr(), g.data_ptr(), f.data_ptr(), *[o.data_ptr() for o in outs],
                             degree_dg=d, stream=stream)

        steps[f"k{k}d{d}_native"] = native
        if d < k - 1:
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                Ge, fe = embed_dg(G, nc, d, k - 1, bs=2), embed_dg(f, nc, d, k - 1)
                t.append((time.perf_counter() - t0) * 1e3)
            host_ms[f"k{k}d{d}"] = float(np.median(t))
            ge_d, fe_d = torch.from_numpy(Ge).to(dev), torch.from_numpy(fe).to(dev)
            keep += [ge_d, fe_d]

            def embedded(k=k, x=x, g=ge_d, f=fe_d):
                cpp.estimate_raw(dm, k, 1, x.data_ptr(), g.data_ptr(), f.data_ptr(), *[o.data_ptr() for o in outs],
                                 stream=stream)

            steps[f"k{k}d{d}_embedded_call"] = embedded
    for fn in steps.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    # clock settle (as bench.py): probes of K steps of every variant, at least 40 ms, until two agree within 1 %
    settle, t0 = [], time.perf_counter()
    while len(settle) < 24:
        tp = time.perf_counter()
        for fn in steps.values():
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
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                steps[name]()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.steps)
    out = {"mesh": f"crossed {args.n}x{args.n}", "ncells": nc, "steps": args.steps, "windows": args.windows,
           "settle_probes": len(settle), "pairs": {}}
    for k, d in pairs:
        v = ms[f"k{k}d{d}_native"]
        med = float(np.median(v))
        row = {"native_ms": med, "min": float(np.min(v)), "max": float(np.max(v)),
               "spread": float((np.max(v) - np.min(v)) / med), "dg_bytes_per_cell": 24 * nd_of(d)}
        if d < k - 1:
            e = ms[f"k{k}d{d}_embedded_call"]
            row.update({"host_embed_ms": host_ms[f"k{k}d{d}"], "embedded_call_ms": float(np.median(e)),
                        "embedded_route_ms": host_ms[f"k{k}d{d}"] + float(np.median(e)),
                        "embedded_dg_bytes_per_cell": 24 * nd_of(k - 1)})
        out["pairs"][f"k{k}d{d}"] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
