"""Cost of a step with new flux boundary values: in-place update against rebuilding the patches.

Two handles at 1M triangles (crossed unit square, n = 500), RT_2:
  stress  stress handle, tractions on the side x = 0 on both rows
  flux    plain flux, prescribed normal flux on the side x = 0
and two routes per step, both in one call of this script:
  update        eqlb_se_update_flux_bc in device memory (point values made by a torch expression at the points of
                eqlb_facet_points; moments + scatter in one launch) + one sweep
  set_boundary  eqlb_se_set_boundary with the dense host array [nrhs][ncells*k(k+2)] + one sweep: the only route
                without the update call
The dense arrays of the second route are built before the clock starts.  Clock settle as in bench.py: W warmup steps,
then untimed probes of K steps for at least 40 ms and until two consecutive ones agree within 1 % (at most 24), then
K timed steps between two synchronisations.  The data are smooth fields plus noise without the compatibility
correction of the tests (the step time does not depend on the values).  Prints one JSON line.

  python tools/bc_update_time.py [--n 500] [--steps 20] [--warmup 3]
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tools"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def settle_and_time(step, sync, steps, warmup):
    for _ in range(warmup):
        step()
    sync()
    probes = []
    t_s0 = time.perf_counter()
    while len(probes) < 24:
        tp = time.perf_counter()
        for _ in range(steps):
            step()
        sync()
        probes.append((time.perf_counter() - tp) / steps * 1e3)
        busy_ms = (time.perf_counter() - t_s0) * 1e3
        if len(probes) >= 2 and busy_ms >= 40.0 and abs(probes[-1] - probes[-2]) <= 0.01 * probes[-2]:
            break
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    sync()
    return (time.perf_counter() - t0) / steps * 1e3, len(probes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    k, nrt, nd = 2, 8, 3

    from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_interval
    from dolfinx_eqlb_amd.mesh import create_unit_square
    from synthetic import dg_points, facet_types
    mesh = create_unit_square(args.n)
    ft1 = facet_types(mesh, lambda p: np.abs(p[:, 0]) < 1e-12)
    facets = np.nonzero(ft1[0] == 2)[0].astype(np.int32)
    rng = np.random.default_rng(7)
    pts = dg_points(mesh, k - 1)
    G1 = np.stack([np.cos(2 * np.pi * pts[..., 0]), np.sin(2 * np.pi * pts[..., 1])], axis=2)
    s, wq = make_quadrature_interval(2 * k)

    import torch
    from dolfinx_eqlb_amd import cpp
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    dm = cpp.DeviceMesh(mesh)
    d_fct = torch.from_numpy(facets).to(dev)
    d_xq = torch.zeros((facets.size, s.size, 2), dtype=torch.float64, device=dev)
    cpp.facet_points_raw(dm, facets.size, d_fct.data_ptr(), s, d_xq.data_ptr(), stream=stream)
    # w(x, y) of the tractions / the flux at the facet points, evaluated on the device
    d_w = torch.stack([1.0 + 0.5 * d_xq[..., 0] - 0.3 * d_xq[..., 1], -0.7 + 0.2 * d_xq[..., 0] + 0.4 * d_xq[..., 1]], -1)
    d_val = torch.empty_like(d_w)
    d_dofs = torch.zeros((facets.size, k), dtype=torch.float64, device=dev)
    cpp.flux_bc_dofs_raw(dm, k, facets.size, d_fct.data_ptr(), s, wq, d_w.data_ptr(), True, d_dofs.data_ptr(),
                         stream=stream)
    torch.cuda.synchronize()
    dofs = d_dofs.cpu().numpy()
    cells = mesh.facet_cells[mesh.facet_cells_offsets[facets]]
    lf = np.argmax(mesh.cell_facets[cells] == facets[:, None], axis=1)
    row = np.zeros(mesh.ncells * nrt)
    for j in range(k):
        row[cells * nrt + lf * k + j] = dofs[:, j]

    out = {"tool": "bc_update_time", "ncells": int(mesh.ncells), "k": k, "bc_facets": int(facets.size),
           "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    for name, nrhs, stress in (("stress", 2, True), ("flux", 1, False)):
        ft = np.repeat(ft1, nrhs, axis=0)
        G = np.stack([G1 + 0.3 * rng.standard_normal(G1.shape) for _ in range(nrhs)]).reshape(nrhs, -1)
        f = rng.standard_normal((nrhs, mesh.ncells * nd))
        d_g, d_f = torch.from_numpy(G).to(dev), torch.from_numpy(f).to(dev)
        d_x = torch.zeros((nrhs, mesh.ncells * nrt), dtype=torch.float64, device=dev)
        # the dense arrays of two alternating steps, built outside the timed region
        dense = [np.ascontiguousarray(np.stack([c * row] * nrhs)) for c in (1.0, 2.0)]
        eq = cpp.SemiExplicitEquilibrator(dm, k, nrhs, reconstruct_stress=stress)
        eq.set_option("accumulate", 0)
        eq.set_boundary(ft, boundary_values=dense[0])
        count = [0]

        def sweep():
            eq.equilibrate_device(d_g.data_ptr(), d_f.data_ptr(), d_x.data_ptr(), stream=stream)

        def step_update():
            count[0] += 1
            torch.mul(d_w, 1.0 + (count[0] % 2), out=d_val)  # the caller's expression for the new values
            for r in range(nrhs):
                eq.update_flux_bc_raw(r, facets.size, d_fct.data_ptr(), d_val.data_ptr(), s, wq, vector=True,
                                      stream=stream)
            sweep()

        def step_set_boundary():
            count[0] += 1
            eq.set_boundary(ft, boundary_values=dense[count[0] % 2])
            sweep()

        ms_sweep, _ = settle_and_time(sweep, torch.cuda.synchronize, args.steps, args.warmup)
        ms_upd, p_upd = settle_and_time(step_update, torch.cuda.synchronize, args.steps, args.warmup)
        eq.check_status(stream)
        table = eq.get_boundary_values()
        expect = dense[count[0] % 2]
        ms_set, p_set = settle_and_time(step_set_boundary, torch.cuda.synchronize, args.steps, args.warmup)
        eq.check_status(stream)
        out[name] = {"sweep_ms": ms_sweep, "update_plus_sweep_ms": ms_upd, "set_boundary_plus_sweep_ms": ms_set,
                     "ratio": ms_set / ms_upd, "settle_probes": [p_upd, p_set],
                     "table_equals_dense_array": bool(np.array_equal(table, expect))}
        eq.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
