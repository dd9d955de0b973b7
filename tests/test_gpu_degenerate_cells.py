"""A cell of zero area on every patch route: reported through check_status, and kept local.

The meshes of tests/degenerate_cases.py hold exactly one cell with det J == 0.0.  Inside a patch kernel its element
matrices are inf and NaN - RT_1 has no pivot that could notice, and the chains of the shuffle solver multiply what they
drag in from the neighbouring patch group by an exact zero, which is no zero for a NaN.  So the set-up finds such cells
(once per mesh), leaves the patches of their three vertices out like masked nodes, and every sweep of the handle raises
the status word.  Each route (options of the handle, i.e. set-up path and kernel instances of the sweep) runs a mesh
once and asserts

  1. reported    a device-memory call followed by check_status raises "patch system not positive definite", the raw C
                 call returns EQLB_ERR_SINGULAR, a second check is clean; a host-memory call on a fresh handle returns
                 the same error;
  2. local       on every cell that shares no vertex with the bad cell the output of the FLAGGED call is finite and
                 equals the oracle summed over exactly the nodes that are not vertices of the bad cell (the
                 unrestricted oracle refuses these meshes, so the reference is assembled node by node; EV: the
                 conforming output in broken form, cell by cell), for every right-hand side;
  3. not sticky  set_boundary on the same handle with a node mask that drops the three vertices, sweep: check_status
                 is clean, ALL cells equal that oracle sum, a second sweep is bitwise equal.

Which instances ran is read from the handle: tiling_blocks() / tiling_info() against the model of tests/tile_classes.py
for the tiled launches (the lists are those of the mask WITHOUT the three vertices, in the flagged run as well),
num_patches, large_patch_info() (the hub of sliver_hub is a vertex of the sliver: nothing is left for the multi-wave
kernels), and the timing slots (option "timing": which patch, weak-symmetry and reduction launches a call recorded)
for the slot routes.

Bounds (relative to the largest coefficient of the reference): 1e-11 for flux, 1e-10 for stress - the oracle bounds of
tests/test_gpu_tile_dispatch.py; 1e-10 at k = 4 (tests/test_gpu_lower_degree.py::_tol, tests/test_gpu_parity.py).  The
large-patch routes: max(that, 10 x the discrepancy recorded for the disk of 70 sectors and two rings), the bound of
tests/test_gpu_large_patches.py.

Data.  Kernels and oracle agree on COMPATIBLE data only (random coefficients differ by 0.8 of the largest coefficient on
a healthy mesh).  The data are made compatible on the mesh WITHOUT the bad cell: it has the same patches at every node
that is not a vertex of the bad cell, so the orthogonality - for stress also the moment balance - holds on every patch
that is compared.  The healthy mesh of the same topology would not do: the cells next to a sliver change shape with it.
The bad cell itself keeps random coefficients.
"""

import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

import degenerate_cases as dc
import tile_classes as tcl

pytestmark = pytest.mark.gpu

EQLB_ERR_SINGULAR = -6     # include/eqlb.h
MESSAGE = "patch system not positive definite"
T_REDUCE, T_WEAKSYM = 5, 6   # timing slots of eqlb_se_last_kernel_ms behind the five bins

Route = namedtuple("Route", "id case kind k nrhs opts deg bc mask env prove")


def R(id, case, kind, k, nrhs=None, opts=(), deg=None, bc="dirichlet", mask=None, env=None, prove=None):
    nrhs = (2 if kind == "stress" else 1) if nrhs is None else nrhs
    return Route(id, case, kind, k, nrhs, tuple(opts), k - 1 if deg is None else deg, bc, mask, env, prove)


def tol(r):
    base = 1e-10 if (r.k == 4 or r.kind == "stress") else 1e-11
    if dict(r.opts).get("large_patches"):
        from test_large_patches_oracle import hub_discrepancy
        base = max(base, 10.0 * hub_discrepancy("disk", 70, 2, r.k))
    return base


# ------------------------------------------------------------------------------------------------ inputs
_SIDES = {"dirichlet": None, "bottom": lambda p: p[:, 1] < 1e-12,
          "strip": lambda p: p[:, 1] < p[:, 1].min() + 0.3 * np.ptp(p[:, 1]),
          "right": lambda p: p[:, 0] > p[:, 0].min() + 0.5 * np.ptp(p[:, 0])}
_ROWS = {"dirichlet": ["dirichlet"] * 3, "flux_bottom": ["bottom"] * 3, "multi": ["dirichlet", "strip", "right"],
         "traction0": ["bottom", "dirichlet"]}


def _types(mesh, bc, nrhs):
    from synthetic import facet_types
    return np.concatenate([facet_types(mesh, _SIDES[s]) for s in _ROWS[bc][:nrhs]])


def _without(mesh, bad):
    from dolfinx_eqlb_amd.mesh import create_mesh
    return create_mesh(mesh.x[:, :2], np.delete(mesh.cell_nodes, bad, axis=0))


_INPUTS = {}


def inputs(case, kind, k, nrhs, deg, bc, offset=0.0):
    """(mesh, bad, facet types, G, f) of a route, built once."""
    key = (case, kind == "stress", k, nrhs, deg, bc, offset)
    if key in _INPUTS:
        return _INPUTS[key]
    from synthetic import make_compatible_data, make_compatible_stress_data
    mesh, bad = dc.case(case, offset)
    nd = (deg + 1) * (deg + 2) // 2
    ft = _types(mesh, bc, nrhs)
    rng = np.random.default_rng(1000 * k + 10 * deg + nrhs)
    G = rng.standard_normal((nrhs, mesh.ncells, nd * 2))     # (what stays of it: the coefficients of the bad cell)
    f = rng.standard_normal((nrhs, mesh.ncells, nd))
    cut = _without(mesh, bad)
    ftc = _types(cut, bc, nrhs)
    keep = np.delete(np.arange(mesh.ncells), bad)
    if kind == "stress":
        Gc, fc = make_compatible_stress_data(cut, k, ftc)
        G[:2, keep] = Gc.reshape(2, cut.ncells, nd * 2)
        f[:2, keep] = fc.reshape(2, cut.ncells, nd)
    else:
        for r in range(nrhs):
            g, ff = make_compatible_data(cut, k, ftc[r:r + 1], degree_dg=deg, seed=17 + r)
            G[r, keep], f[r, keep] = g.reshape(cut.ncells, -1), ff.reshape(cut.ncells, -1)
    out = (mesh, bad, ft, np.ascontiguousarray(G.reshape(nrhs, -1)), np.ascontiguousarray(f.reshape(nrhs, -1)))
    _INPUTS[key] = out
    return out


_REFS = {}


def reference(oracle_mod, key, mesh, kind, k, deg, ft, G, f, mask):
    """Oracle summed over the nodes of `mask`, in the broken per-cell layout [nrhs, ncells, nrt]; computed once."""
    key = key + (mask.tobytes(),)
    if key not in _REFS:
        nrt = k * (k + 2)
        if kind == "ev":
            from dolfinx_eqlb_amd.eqlb.conforming import conforming_dofmap, conforming_to_broken
            cd, nd = conforming_dofmap(mesh, k)
            ref = np.zeros((G.shape[0], nd))
            for node in np.nonzero(mask)[0]:
                oracle_mod.ev_reconstruct(mesh, k, ft, G, f, cd, nd, flux_hdiv=ref, node_range=(int(node), int(node) + 1))
            ref = np.stack([conforming_to_broken(mesh, k, r) for r in ref])
        else:
            ref = np.zeros((G.shape[0], mesh.ncells * nrt))
            for node in np.nonzero(mask)[0]:
                oracle_mod.se_reconstruct(mesh, k, ft, G, f, degree_dg=deg, flux_hdiv=ref,
                                          node_range=(int(node), int(node) + 1), stress=(kind == "stress"))
        assert np.isfinite(ref).all()
        ref = ref.reshape(G.shape[0], mesh.ncells, nrt)
        ref.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


# ------------------------------------------------------------------------------------------------ handles
@pytest.fixture(scope="module")
def cpp():
    from dolfinx_eqlb_amd import cpp as c
    assert c.device_count() >= 1, "GPU tests need a HIP device"
    return c


def make_handle(cpp, dm, r, ft, mask):
    if r.kind == "ev":
        eq = cpp.ConstrainedMinEquilibrator(dm, r.k, r.nrhs, degree_dg=r.deg)
    else:
        eq = cpp.SemiExplicitEquilibrator(dm, r.k, r.nrhs, degree_dg=r.deg, reconstruct_stress=(r.kind == "stress"))
    for key, value in r.opts:
        eq.set_option(key, value)
    eq.set_boundary(ft, node_mask=mask)
    return eq


class Device:
    """The arrays of one route in device memory, and sweeps on them."""

    def __init__(self, cpp, mesh, r, G, f):
        import torch
        self.torch, self.cpp, self.mesh, self.r = torch, cpp, mesh, r
        self.dev = torch.device("cuda", 0)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.G, self.f = torch.from_numpy(G).to(self.dev), torch.from_numpy(f).to(self.dev)

    def sweep(self, eq):
        """One device-memory call from zeros; the result in the broken layout [nrhs, ncells, nrt] - read back after the
        caller has looked at the status."""
        r, nrt = self.r, self.r.k * (self.r.k + 2)
        nout = eq.ndofs if r.kind == "ev" else self.mesh.ncells * nrt
        x = self.torch.zeros(r.nrhs * nout, dtype=self.torch.float64, device=self.dev)
        eq.equilibrate_device(self.G.data_ptr(), self.f.data_ptr(), x.data_ptr(), self.stream)
        return x

    def status(self, eq):
        """The raw C call: (return code, message)."""
        lib = self.cpp.lib()
        fn = lib.eqlb_ev_check_status if self.r.kind == "ev" else lib.eqlb_se_check_status
        rc = fn(eq._h, C.c_void_p(self.stream))
        return rc, (lib.eqlb_last_error().decode() if rc else "")

    def broken(self, x):
        r, nrt = self.r, self.r.k * (self.r.k + 2)
        x = x.cpu().numpy().reshape(r.nrhs, -1)
        if r.kind == "ev":
            from dolfinx_eqlb_amd.eqlb.conforming import conforming_to_broken
            x = np.stack([conforming_to_broken(self.mesh, r.k, row) for row in x])
        return x.reshape(r.nrhs, self.mesh.ncells, nrt)


def check_local(r, x, ref, cells, what):
    """x == ref on `cells`, every right-hand side, every value finite; returns the largest relative deviation."""
    worst = 0.0
    for rhs in range(r.nrhs):
        scale = np.abs(ref[rhs]).max()
        assert scale > 0.0
        got = x[rhs][cells]
        assert np.isfinite(got).all(), f"{r.id}: {what}, rhs {rhs}: non-finite values away from the bad cell"
        err = np.abs(got - ref[rhs][cells]).max() / scale
        assert err <= tol(r), f"{r.id}: {what}, rhs {rhs}: {err:.3e} of the largest coefficient (bound {tol(r):.0e})"
        worst = max(worst, err)
    return worst


def run_route(cpp, oracle_mod, monkeypatch, r):
    for name, value in (r.env or {}).items():
        monkeypatch.setenv(name, value)
    mesh, bad, ft, G, f = inputs(r.case, r.kind, r.k, r.nrhs, r.deg, r.bc)
    good = dc.good_mask(mesh, bad)
    mask = np.ones(mesh.nnodes, np.uint8) if r.mask is None else r.mask(mesh, bad)
    assert mask[mesh.cell_nodes[bad]].all()      # the bad patches are part of the run
    far = dc.far_cells(mesh, bad)
    key = (r.case, r.kind, r.k, r.nrhs, r.deg, r.bc)
    ref = reference(oracle_mod, key, mesh, r.kind, r.k, r.deg, ft, G, f, mask & good)
    dm = cpp.DeviceMesh(mesh)
    dv = Device(cpp, mesh, r, G, f)

    eq = make_handle(cpp, dm, r, ft, mask)
    if r.prove:
        r.prove(eq, mesh, mask & good, r)
    # 1. reported
    x = dv.sweep(eq)
    with pytest.raises(RuntimeError, match=MESSAGE):
        eq.check_status(dv.stream)
    eq.check_status(dv.stream)
    x_again = dv.sweep(eq)
    assert dv.status(eq) == (EQLB_ERR_SINGULAR, MESSAGE)
    assert dv.status(eq) == (0, "")
    fresh = make_handle(cpp, dm, r, ft, mask)
    with pytest.raises(RuntimeError, match=MESSAGE):
        fresh.equilibrate_host(G, f)
    fresh.close()
    # 2. local (both flagged calls)
    e_local = check_local(r, dv.broken(x), ref, far, "flagged call")
    check_local(r, dv.broken(x_again), ref, far, "second flagged call")
    # 3. not sticky, not lost
    eq.set_boundary(ft, node_mask=mask & good)
    x1 = dv.sweep(eq)
    eq.check_status(dv.stream)
    x2 = dv.sweep(eq)
    eq.check_status(dv.stream)
    assert bool((x1 == x2).all())
    e_all = check_local(r, dv.broken(x1), ref, np.arange(mesh.ncells), "masked call")
    if r.prove:
        r.prove(eq, mesh, mask & good, r, after=True)
    print(f"{r.id}: local {e_local:.2e}, masked {e_all:.2e} (bound {tol(r):.0e})")
    eq.close()


# ------------------------------------------------------------------------------------------------ proofs
FULL = 0   # class of a full patch in tests/tile_classes.py


def tiled(stress=False, mixed=False):
    """The handle runs one tile whose wave-blocks are the predicted ones - those of the mask without the vertices of the
    bad cell, in the flagged run as well: the set-up leaves their patches out."""
    def prove(eq, mesh, mask, r, after=False):
        tb = eq.tiling_blocks()
        assert tb == tcl.predict(mesh, r.k, mask, stress, mixed), (tb, tcl.predict(mesh, r.k, mask, stress, mixed))
        if r.kind != "ev":
            info = eq.tiling_info()
            assert info["ntiles"] == 1 and info["patch_instances"] == tcl.patch_instances(mesh, mask, stress, mixed)
        assert tb["zero_tiles"] == 1     # (nodes without a patch: rows that are never written)
    return prove


def slots(bins, fused=False, weaksym=False, large=None):
    """Slot route: the reduction ran; per-bin launches (one timing slot per bin) or the launch of all bins at once (slot
    of bin 0 alone); the weak-symmetry launches.  large: large_patch_info() of the handle - the hub of sliver_hub is a
    vertex of the bad cell, so the multi-wave kernel has nothing to do.  Read after the sweeps."""
    def prove(eq, mesh, mask, r, after=False):
        assert large is None or eq.large_patch_info() == large
        assert eq.num_patches == int(mask.sum())
        if not after:
            return
        assert eq.last_kernel_ms(T_REDUCE) > 0.0
        for b in bins:
            assert (eq.last_kernel_ms(b) > 0.0) == (b == 0 or not fused), (b, fused)
        assert (eq.last_kernel_ms(T_WEAKSYM) > 0.0) == weaksym
    return prove


def tiled_large(large):
    def prove(eq, mesh, mask, r, after=False):
        assert eq.large_patch_info() == large
        assert eq.tiling_blocks()["zero_tiles"] >= 1
    return prove


def full8_mask(n):
    """Node mask with n healthy full 8-cell patches and the three patches of the bad cell, nothing else."""
    def make(mesh, bad):
        b, c = tcl.node_bins_classes(mesh)
        full8 = np.nonzero((b == 1) & (c == FULL))[0]
        mine = [v for v in mesh.cell_nodes[bad] if v in full8]
        assert len(mine) == 2
        rest = [v for v in full8 if v not in mine]
        mask = np.zeros(mesh.nnodes, np.uint8)
        mask[mine + rest[:n]] = 1
        mask[[v for v in mesh.cell_nodes[bad] if v not in mine]] = 1   # (the full 4-cell patch of the bad cell)
        return mask
    return make


# ------------------------------------------------------------------------------------------------ routes
TIMED = (("timing", 1),)


def _routes():
    out = []
    # flux, SE: tiled launch, RT_1 ... RT_3, automatic and explicit choice
    for case, bc in (("collapsed", "dirichlet"), ("sliver", "dirichlet"), ("sliver_boundary", "dirichlet"),
                     ("sliver_boundary", "flux_bottom")):
        for k in (1, 2, 3):
            for sc in (-1, 2):
                out.append(R(f"se-tiled-{case}-{bc}-k{k}-sc{sc}", case, "se", k, opts=[("scatter", sc)], bc=bc,
                             prove=tiled()))
    # RT_2, the two bad full 8-cell patches next to 16 healthy ones (a whole pair-lane wave-block: two 64-lane blocks of
    # full patches) | next to 15 and 8 (the lane = cell full-patch instance, one block)
    for n, full, generic in ((16, 2, 0), (15, 1, 1), (8, 1, 0)):
        def prove(eq, mesh, mask, r, after=False, full=full, generic=generic):
            tiled()(eq, mesh, mask, r, after)
            tb = eq.tiling_blocks()
            assert (tb["full"][1], tb["interior"][1], tb["generic"][1]) == (full, 0, generic), tb
            assert sum(tb["full"]) + sum(tb["generic"]) == full + generic      # (nothing in the other bins)
        out.append(R(f"se-tiled-collapsed-k2-full8x{n}", "collapsed", "se", 2, mask=full8_mask(n), prove=prove))
    # slot path: the launch of all bins at once ("fused" with the shuffle solver) | one launch per bin
    for case, bins in (("collapsed", (0, 1)), ("sliver", (0, 1))):
        for k in (1, 2, 3):
            for fused in (0, 1):
                for solver in (0, 1):
                    out.append(R(f"se-slots-{case}-k{k}-fused{fused}-solver{solver}", case, "se", k,
                                 opts=[("scatter", 0), ("fused", fused), ("solver", solver)] + list(TIMED),
                                 prove=slots(bins, fused=bool(fused and solver))))
    # RT_4: per-bin launches
    for case, bins in (("collapsed", (0, 1)), ("sliver", (0, 1))):
        for solver in (0, 1):
            out.append(R(f"se-k4-{case}-solver{solver}", case, "se", 4, opts=[("solver", solver)] + list(TIMED),
                         prove=slots(bins)))
    # several right-hand sides with different facet types in one tiled launch
    for k in (2, 3):
        for nrhs in (2, 3):
            out.append(R(f"se-multi-k{k}-r{nrhs}", "collapsed", "se", k, nrhs=nrhs, opts=[("multi_rhs", 1)], bc="multi",
                         prove=tiled()))
    # data of a lower degree: one pair per translation unit
    for k, d in ((2, 0), (3, 1), (3, 0)):
        out.append(R(f"se-lowdeg-k{k}-d{d}", "collapsed", "se", k, deg=d, prove=tiled()))
    for d in (2, 1, 0):
        out.append(R(f"se-lowdeg-k4-d{d}", "collapsed", "se", 4, deg=d, opts=TIMED, prove=slots((0, 1))))
    # the hub of 71 cells on the multi-wave kernel
    for k in (1, 2, 3, 4):
        out.append(R(f"se-large-k{k}-slots", "sliver_hub", "se", k, opts=[("large_patches", 1), ("scatter", 0)] + list(TIMED),
                     prove=slots((), large=(0, 0))))
        if k <= 3:
            out.append(R(f"se-large-k{k}-tiled", "sliver_hub", "se", k, opts=[("large_patches", 1), ("scatter", 2)],
                         prove=tiled_large((0, 0))))
    # flux, EV
    for case in ("collapsed", "sliver"):
        for k in (1, 2, 3):
            out.append(R(f"ev-tiled-{case}-k{k}", case, "ev", k, prove=tiled()))
        bins = (0, 1)
        out.append(R(f"ev-fused-{case}-k3", case, "ev", 3, opts=[("scatter", 0)] + list(TIMED),
                     prove=slots(bins, fused=True)))
        out.append(R(f"ev-slots-{case}-k4", case, "ev", 4, opts=TIMED, prove=slots(bins)))
    out.append(R("ev-large-k2", "sliver_hub", "ev", 2, opts=[("large_patches", 1)], prove=tiled_large((0, 0))))
    # stress: fused launch with lists of full patches only | with every patch of up to 8 lanes
    out.append(R("stress-fused-full-collapsed", "collapsed", "stress", 2, env={"EQLB_STRESS_MIXED_TILES": "0"},
                 prove=tiled(True, False)))
    for case in ("collapsed", "sliver", "sliver_boundary"):
        out.append(R(f"stress-fused-mixed-{case}", case, "stress", 2, env={"EQLB_STRESS_MIXED_TILES": "1"},
                     prove=tiled(True, True)))
    # slot route: k_se_weaksym_lean | k_se_weaksym<2, P> (tractions on one row) | k_se_weaksym<K, P> | banded
    out.append(R("stress-slots-lean-collapsed", "collapsed", "stress", 2, opts=[("scatter", 0)] + list(TIMED),
                 prove=slots((0, 1), fused=True, weaksym=True)))
    out.append(R("stress-slots-traction-collapsed", "collapsed", "stress", 2, opts=[("scatter", 0)] + list(TIMED),
                 bc="traction0", prove=slots((0, 1), fused=True, weaksym=True)))
    for k in (3, 4):
        out.append(R(f"stress-slots-collapsed-k{k}", "collapsed", "stress", k, opts=TIMED,
                     prove=slots((0, 1), fused=(k == 3), weaksym=True)))
    out.append(R("stress-banded-sliver-k4", "sliver", "stress", 4, opts=TIMED, prove=slots((0, 1), weaksym=True)))
    out.append(R("stress-banded-hub40-k3", "sliver_hub40", "stress", 3, opts=TIMED,
                 prove=slots((0, 1), fused=True, weaksym=True)))
    for k in (2, 3, 4):
        out.append(R(f"stress-large-k{k}", "sliver_hub", "stress", k,
                     opts=[("large_patches", 1), ("large_patches_stress", 1), ("scatter", 0)] + list(TIMED),
                     prove=slots((), weaksym=True, large=(0, 0))))
    out.append(R("stress-large-k2-tiled", "sliver_hub", "stress", 2,
                 opts=[("large_patches", 1), ("large_patches_stress", 1)], prove=tiled_large((0, 0))))
    return out


ROUTES = _routes()


def test_route_table_is_complete():
    ids = [r.id for r in ROUTES]
    assert len(set(ids)) == len(ids)
    assert all(dc.case(r.case)[0].ncells <= 260 for r in ROUTES)


@pytest.mark.parametrize("route", ROUTES, ids=[r.id for r in ROUTES])
def test_zero_area_cell_is_reported_and_stays_local(cpp, oracle_mod, monkeypatch, route):
    run_route(cpp, oracle_mod, monkeypatch, route)


# ------------------------------------------------------------------------------------------------ towards the limit
LIMIT_ROUTES = [R("se-k2", "collapsed", "se", 2), R("se-k3", "collapsed", "se", 3), R("stress-k2", "collapsed", "stress", 2)]


@pytest.mark.parametrize("offset", dc.LIMIT_OFFSETS, ids=["2^-10", "2^-26", "2^-52"])
@pytest.mark.parametrize("route", LIMIT_ROUTES, ids=[r.id for r in LIMIT_ROUTES])
def test_nearly_flat_cell(cpp, oracle_mod, route, offset):
    """The centre node `offset` of the square's width off the edge: whatever the conditioning, the run is flagged or
    every value is finite, and the cells away from the sliver get the oracle's values either way.  No accuracy is
    asserted on the cells that touch the sliver (the table of DESIGN.md 8(f)-4 records what was observed)."""
    r = route
    mesh, bad, ft, G, f = inputs(r.case, r.kind, r.k, r.nrhs, r.deg, r.bc, offset)
    good = dc.good_mask(mesh, bad)
    ref = reference(oracle_mod, (r.id, offset), mesh, r.kind, r.k, r.deg, ft, G, f, good)
    dv = Device(cpp, mesh, r, G, f)
    eq = make_handle(cpp, cpp.DeviceMesh(mesh), r, ft, None)
    x = dv.sweep(eq)
    rc, msg = dv.status(eq)
    x = dv.broken(x)
    finite = bool(np.isfinite(x).all())
    print(f"{r.id} offset {offset:.1e}: " + ("flagged" if rc else "clean")
          + (f", largest value {np.abs(x).max():.3e}" if finite else ", non-finite values"))
    assert rc in (0, EQLB_ERR_SINGULAR) and (rc == 0 or msg == MESSAGE)
    assert rc == EQLB_ERR_SINGULAR or finite
    check_local(r, x, ref, dc.far_cells(mesh, bad), "nearly flat cell")
    eq.close()
