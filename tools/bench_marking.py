#!/usr/bin/env python3
"""Time eqlb_mark_doerfler on device-resident indicators against the host route of the reference's adaptive demos.

  python tools/bench_marking.py [--sizes 1000000 8000000] [--theta 0.5] [--steps 20] [--warmup 3] [--windows 5]

Indicators: np.random.default_rng(0).lognormal(0, 2, ncells), device resident.  Per size
  device call   cpp.mark_doerfler_raw through the C ABI on device memory (torch's current stream), HIP events:
                after the warm-up and the clock-settle probes of bench.py (probes of K calls for at least 40 ms until
                two agree within 1 %), `--windows` windows of K calls each; mean over all windows x K calls (100
                with the defaults), min and max over the windows
  host route    in the same process: device-to-host copy of the indicators (torch .cpu(), wall time around a
                synchronise) plus eqlb.doerfler_marking (numpy: stable argsort, cumsum, sort of the marked ids);
                median of 5 runs each
and the check that both give the same list.  Also the time of eqlb_indicator_total (two terms, pair_last_two) on
the same windows.  Prints one JSON object.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 8_000_000])
    ap.add_argument("--theta", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()

    import torch  # first: its HIP runtime is the one the library binds to (bench.py)
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.eqlb import doerfler_marking

    dev = torch.device("cuda:0")
    torch.cuda.init()
    stream = torch.cuda.current_stream().cuda_stream
    out = {"theta": args.theta, "steps": args.steps, "windows": args.windows, "sizes": {}}
    for n in args.sizes:
        eta = np.random.default_rng(0).lognormal(0, 2, n)
        eta_d = torch.from_numpy(eta).to(dev)
        osc_d = torch.from_numpy(np.random.default_rng(1).lognormal(0, 2, n)).to(dev)
        marked = torch.empty(n, dtype=torch.int32, device=dev)
        nm = torch.zeros(1, dtype=torch.int64, device=dev)
        tot = torch.zeros(3, dtype=torch.float64, device=dev)
        cell = torch.empty(n, dtype=torch.float64, device=dev)

        def mark():
            cpp.mark_doerfler_raw(n, eta_d.data_ptr(), args.theta, marked.data_ptr(), nm.data_ptr(), tot.data_ptr(),
                                  stream=stream)

        def indicator():
            cpp.indicator_total_raw(n, [eta_d.data_ptr(), osc_d.data_ptr()], True, cell.data_ptr(), tot.data_ptr(),
                                    stream=stream)

        steps = {"mark_doerfler": mark, "indicator_total": indicator}
        for fn in steps.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
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
            for name in (names if w % 2 == 0 else names[::-1]):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.steps):
                    steps[name]()
                e1.record()
                torch.cuda.synchronize()
                ms[name].append(e0.elapsed_time(e1) / args.steps)
        mark()
        torch.cuda.synchronize()
        nmarked = int(nm.item())
        got = marked[:max(nmarked, 0)].cpu().numpy()
        # the host route
        d2h, host = [], []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h = eta_d.cpu().numpy()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            ref = doerfler_marking(h, args.theta)
            t2 = time.perf_counter()
            d2h.append((t1 - t0) * 1e3)
            host.append((t2 - t1) * 1e3)
        row = {"nmarked": nmarked, "same_list_as_host": bool(np.array_equal(got, ref)), "settle_probes": len(settle),
               "d2h_copy_ms": float(np.median(d2h)), "host_doerfler_marking_ms": float(np.median(host)),
               "host_route_ms": float(np.median(d2h) + np.median(host))}
        for name, v in ms.items():
            row[name + "_ms"] = float(np.mean(v))
            row[name + "_min"] = float(np.min(v))
            row[name + "_max"] = float(np.max(v))
        out["sizes"][str(n)] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
