#!/usr/bin/env python3
"""Time eqlb_primal_flux_dg / eqlb_primal_stress_dg with a device-resident solution on the 1M-triangle crossed mesh.

  python tools/bench_primal_flux.py [--n 500] [--pairs 2,1 1,1 3,2] [--steps 20] [--warmup 3] [--windows 5]

Per pair (p, d) the flux call, plus the stress call at (2, 1), through the C ABI on device memory (torch's current
stream): one kernel per call, nothing else, timed with HIP events.  Next to each time:
  host_route_ms     what the same result costs without the entry point: the numpy statement of
                    tests/galerkin.py::discrete_flux on the host (wall time, median of 3) plus the upload of its
                    result (timed with events from pinned memory);
  bytes_per_cell    the bytes the algorithm needs per cell: index row 4 nd_p + J 32 + output 16 nd_d per row
                    (+ 8 for a cell-wise coefficient: none here) + the unique DOFs 8 ndofs / ncells per solution row;
  roofline_fraction bytes_per_cell * ncells / 8 TB/s over the measured time.
k_project_dg (eqlb_project_dg, DG_1, bs = 2, the 9 points of the degree-4 rule: 144 B in, 48 B out per cell) runs in
the same windows as the comparable streaming kernel; its call uploads its matrix and waits for the stream, so its
event time is an upper bound of its kernel time (the kernel trace of a profiler run separates the two).
All variants run in one process after the warm-up and the clock-settle probes of bench.py (probes of K steps for at
least 40 ms until two agree within 1 %), then in alternating order in `--windows` windows of K steps each.  Prints one
JSON object.
"""

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK_BYTES_PER_S = 8.0e12


def nd_of(d):
    return (d + 1) * (d + 2) // 2


def dofmap(mesh, k):
    """Cell dofmap of the conforming P_k space: vertices, k-1 DOFs per edge along the global edge direction, then the
    cell-interior DOFs (the numbering of elmtlib/lagrange.py)."""
    nn, nf, nc = mesh.nnodes, mesh.nfacets, mesh.ncells
    ne, ni = k - 1, (k - 1) * (k - 2) // 2
    cd = np.empty((nc, (k + 1) * (k + 2) // 2), dtype=np.int32)
    cd[:, :3] = mesh.cell_nodes
    col = 3
    for f in range(3):
        base = nn + mesh.cell_facets[:, f].astype(np.int64) * ne
        for j in range(ne):
            cd[:, col] = base + np.where(mesh.facet_perm[:, f] == 1, ne - 1 - j, j)
            col += 1
    for j in range(ni):
        cd[:, col] = nn + nf * ne + np.arange(nc, dtype=np.int64) * ni + j
        col += 1
    return cd, nn + nf * ne + nc * ni


def host_flux(mesh, K, PG, u, cd):
    """The numpy statement of discrete_flux for one solution vector."""
    gref = np.einsum("ci,Xni->cnX", u[cd], PG)
    return np.ascontiguousarray(-np.einsum("cXd,cnX->cnd", K, gref).reshape(-1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--pairs", nargs="+", default=["2,1", "1,1", "3,2"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    pairs = [tuple(int(v) for v in p.split(",")) for p in args.pairs]

    import torch  # first: its HIP runtime is the one the library binds to (bench.py)
    from dolfinx_eqlb_amd import cpp
    from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
    from dolfinx_eqlb_amd.eqlb.check_eqlb_conditions import cell_geometry
    from dolfinx_eqlb_amd.mesh import create_unit_square

    dev = torch.device("cuda:0")
    torch.cuda.init()
    mesh = create_unit_square(args.n, shuffle_seed=1234)
    dm = cpp.DeviceMesh(mesh)
    nc = mesh.ncells
    K = cell_geometry(mesh)[2]
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(0)
    steps, info, keep = {}, {}, []

    def add(name, p, d, stress):
        cd, ndofs = dofmap(mesh, p)
        rows = 2 if stress else 1
        u = rng.standard_normal((ndofs, 2)) if stress else rng.standard_normal(ndofs)
        cd_d, u_d = torch.from_numpy(cd).to(dev), torch.from_numpy(u).to(dev)
        out = torch.empty(rows * nc * nd_of(d) * 2, dtype=torch.float64, device=dev)
        keep.extend([cd_d, u_d, out])
        if stress:
            def fn():
                cpp.primal_stress_dg_raw(dm, p, d, cd_d.data_ptr(), ndofs, u_d.data_ptr(), 1.0, None, out.data_ptr(),
                                         stream=stream)
        else:
            def fn():
                cpp.primal_flux_dg_raw(dm, p, d, 1, cd_d.data_ptr(), ndofs, u_d.data_ptr(), None, out.data_ptr(),
                                       stream=stream)
        steps[name] = fn
        # the host route: numpy statement + upload of its result
        PG = cpp.get_primal_table(p, d)
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            if stress:
                uc = u[cd]                                           # [c, i, r]
                gu = np.einsum("cXd,Xni,cir->cnrd", K, PG, uc)
                sig = gu + np.swapaxes(gu, 2, 3)
                div = gu[..., 0, 0] + gu[..., 1, 1]
                sig[..., 0, 0] += div
                sig[..., 1, 1] += div
                G = np.stack([np.ascontiguousarray(-sig[:, :, r, :].reshape(-1)) for r in range(2)])
            else:
                G = host_flux(mesh, K, PG, u, cd)
            t.append((time.perf_counter() - t0) * 1e3)
        pinned = torch.from_numpy(G.reshape(-1)).pin_memory()
        up = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out.copy_(pinned, non_blocking=True)
            e1.record()
            torch.cuda.synchronize()
            up.append(e0.elapsed_time(e1))
        bpc = 4 * nd_of(p) + 32 + rows * 16 * nd_of(d) + rows * 8.0 * ndofs / nc
        info[name] = {"p": p, "d": d, "stress": stress, "ndofs": ndofs, "host_numpy_ms": float(np.median(t)),
                      "upload_ms": float(np.median(up)), "bytes_per_cell": bpc}

    for p, d in pairs:
        add(f"p{p}d{d}_flux", p, d, False)
    add("p2d1_stress", 2, 1, True)

    # the comparable streaming kernel of the project
    qp, qw = [np.ascontiguousarray(a, dtype=np.float64) for a in make_quadrature_triangle(4)]
    nq = qw.size
    qv = torch.from_numpy(rng.standard_normal(nc * nq * 2)).to(dev)
    pout = torch.empty(nc * 3 * 2, dtype=torch.float64, device=dev)
    keep.extend([qv, pout])

    def project():
        cpp._check(cpp.lib().eqlb_project_dg(dm._h, C.c_int32(1), C.c_int32(2), C.c_int32(1), C.c_int32(nq),
                                             cpp._hp(qp), cpp._hp(qw), C.c_void_p(qv.data_ptr()),
                                             C.c_void_p(pout.data_ptr()), C.c_int32(cpp.MEM_DEVICE),
                                             C.c_void_p(stream)))

    steps["project_dg_d1_bs2"] = project
    info["project_dg_d1_bs2"] = {"bytes_per_cell": 8.0 * 2 * (nq + 3), "nq": int(nq)}

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
           "settle_probes": len(settle), "peak_bytes_per_s": PEAK_BYTES_PER_S, "calls": {}}
    for name in names:
        v = ms[name]
        med = float(np.median(v))
        row = dict(info[name])
        row.update({"ms": med, "min": float(np.min(v)), "max": float(np.max(v)),
                    "spread": float((np.max(v) - np.min(v)) / med),
                    "roofline_fraction": row["bytes_per_cell"] * nc / PEAK_BYTES_PER_S / (med * 1e-3)})
        if "host_numpy_ms" in row:
            row["host_route_ms"] = row["host_numpy_ms"] + row["upload_ms"]
        out["calls"][name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
