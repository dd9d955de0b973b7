"""The estimator kernels value by value against the float64 statements of tests/estimator_cases.py, on its table of hard
meshes and launch shapes: |device - statement| <= c 2^-53 A per value, c and A as derived there (the statement alone stays
within half of that against long double, tests/test_estimator_statements_host.py).  The Korn constants are held against
the oracle within the tolerance that the conditioning of 2 / sin^2(theta / 2) gives.  Every test prints its largest
|device - statement| / bound.

Largest ratios measured on the MI355X, per quantity (mesh, k-d): see README, "Tests"."""

import ctypes as C

import numpy as np
import pytest

import estimator_cases as E

pytestmark = pytest.mark.gpu

CASES = E.CASES + [(n, k, d) for n in E.LOWDEG_MESHES_GPU for k, d in E.LOWDEG]
STRESS_CASES = [(n, k) for n in E.MESHES for k in (1, 2, 3, 4)]
NRHS = 3


@pytest.fixture(scope="module")
def cpp():
    from dolfinx_eqlb_amd import cpp as c
    assert c.device_count() >= 1, "GPU tests need a HIP device"
    E.check_table()
    return c


_DM = {}


def device_mesh(cpp, name):
    if name not in _DM:
        _DM[name] = cpp.DeviceMesh(E.mesh_of(name))
    return _DM[name]


def held(label, key, got, val, A, c, worst, where=None):
    """asserts |got - val| <= c U A value by value and records the largest ratio"""
    assert np.all(np.isfinite(got)), (label, key)
    diff, bound = E.deviation(key, got, val, A, c)
    r = E.ratio(diff, bound)
    worst[key] = max(worst.get(key, 0.0), r)
    bad = np.nonzero(~(diff <= bound))[0]
    note = "" if where is None or bad.size == 0 else " " + where(bad)
    assert bad.size == 0, f"{label} {key}: {bad.size} values outside the bound, largest ratio {r:.3f}, first at " \
                          f"{bad[:5].tolist()}{note}"


def report(label, worst):
    print(f"{label}: max |device - statement| / bound: " + " ".join(f"{q}={v:.3f}" for q, v in worst.items()))


def deg_arg(k, d):
    return None if d == k - 1 else d      # the entry points without _dg at d = k - 1


# ------------------------------------------------------------------------------------------------------ cpp.estimate
@pytest.mark.parametrize("case", CASES, ids=E.case_id)
def test_estimate_per_cell_and_facet(cpp, case):
    name, k, d = case
    mesh, D, dm = E.mesh_of(name), E.data(name, k, d), device_mesh(cpp, name)
    q = [E.quantities(name, k, d, r=r, stress=False) for r in range(NRHS)]
    bnd = np.diff(mesh.facet_cells_offsets) == 1
    worst = {}
    for ev in (False, True):
        tag = "_ev" if ev else ""
        for nrhs in (1, NRHS):
            got = cpp.estimate(dm, k, D["x"][:nrhs], D["G"][:nrhs], D["f"][:nrhs], conforming_flux=ev,
                               degree_dg=deg_arg(k, d))
            for r in range(nrhs):
                for key, g in zip(("div2", "sig2", "jump"), got):
                    held(f"{E.case_id(case)} nrhs={nrhs} r={r}", key + tag, g[r], *q[r][key + tag], worst)
                assert np.all(got[2][r][bnd] == 0.0) and np.all(got[2][r][~bnd] > 0.0)
    report(E.case_id(case), worst)


# --------------------------------------------------------------------------------------------------- cpp.oscillation
@pytest.mark.parametrize("case", CASES, ids=E.case_id)
def test_oscillation_per_cell(cpp, case):
    name, k, d = case
    D, dm = E.data(name, k, d), device_mesh(cpp, name)
    q = [E.quantities(name, k, d, r=r, stress=False) for r in range(NRHS)]
    worst = {}
    for key, (with_g, with_korn) in E.OSC.items():
        for nrhs in (1, NRHS):
            got = cpp.oscillation(dm, k, D["x"][:nrhs], D["G"][:nrhs] if with_g else None, D["qp"], D["qw"],
                                  D["fv"][:nrhs], D["korn"] if with_korn else None, degree_dg=deg_arg(k, d))
            for r in range(nrhs):
                held(f"{E.case_id(case)} nrhs={nrhs} r={r}", key, got[r], *q[r][key], worst)
                assert np.all(got[r] > 0.0)
    report(E.case_id(case), worst)


# --------------------------------------------------------------------------------------------- cpp.boundary_residual
@pytest.mark.parametrize("case", CASES, ids=E.case_id)
def test_boundary_residual_per_facet(cpp, case):
    name, k, d = case
    D, dm = E.data(name, k, d), device_mesh(cpp, name)
    facets = D["facets"]
    q = [E.quantities(name, k, d, r=r, stress=False) for r in range(NRHS)]
    args = {"bres": (True, False), "bres_bv": (True, True), "bres_sigma": (False, True)}
    # sq33: lists of one entry, of a workgroup less one, a whole one and one more.  Its boundary has 132 facets only, so
    # the lists are cut from the boundary list walked round and round (a facet may be listed twice), from entry 3 on.
    lengths = [facets.size] + ([1, 255, 256, 257] if name == "sq33" else [])
    worst = {}
    for key, (with_g, with_bv) in args.items():
        for n in lengths:
            for nrhs in ((1, NRHS) if n == facets.size else (NRHS,)):
                pick = np.arange(n) if n == facets.size else (3 + np.arange(n)) % facets.size
                got = cpp.boundary_residual(dm, k, D["x"][:nrhs], D["G"][:nrhs] if with_g else None, facets[pick],
                                            D["bv"][:nrhs] if with_bv else None, degree_dg=d)
                assert got.shape == (nrhs, n)
                for r in range(nrhs):
                    val, A, c = q[r][key]
                    held(f"{E.case_id(case)} n={n} nrhs={nrhs} r={r}", key, got[r], val[pick], A[pick], c, worst)
    report(E.case_id(case), worst)


# ----------------------------------------------------------------------------------------------- cpp.estimate_stress
def special_nodes(name, mesh):
    """the nodes a wrong vertex sum would show at: label -> node numbers"""
    import topology_meshes as tm
    if name == "disk100":
        return {"hub of 100 cells": np.nonzero(np.diff(mesh.node_cells_offsets) == 100)[0]}
    if name == "hole":
        return {"inner loop": np.unique(mesh.facet_nodes[tm.inner_loop_facets(mesh)])}
    if name == "bowtie":
        return {"pinched vertex": np.array([tm.pinched_node(mesh)])}
    return {}


@pytest.mark.parametrize("case", STRESS_CASES, ids=E.case_id)
def test_estimate_stress_per_cell_and_node(cpp, case):
    name, k = case
    mesh, D, dm = E.mesh_of(name), E.data(name, k, k - 1), device_mesh(cpp, name)
    special = special_nodes(name, mesh)
    assert all(v.size > 0 for v in special.values())

    def where(bad):
        hit = [f"{label} (nodes {np.intersect1d(bad, v).tolist()})" for label, v in special.items()
               if np.intersect1d(bad, v).size]
        if hit:
            return "among them: " + ", ".join(hit)
        return ("none of them at: " + ", ".join(special)) if special else ""
    worst = {}
    for r in range(2):                                        # rows (0, 1) and (1, 2) of the data as the two stress rows
        q = E.quantities(name, k, k - 1, r=r)
        x2 = D["x"][r:r + 2]
        for p in E.PI_1:
            energy, wsym, asym = cpp.estimate_stress(dm, k, x2, D["korn"], p)
            held(f"{E.case_id(case)} r={r}", f"energy{p:g}", energy, *q[f"energy{p:g}"], worst)
            held(f"{E.case_id(case)} r={r}", f"wsym{p:g}", wsym, *q[f"wsym{p:g}"], worst)
            held(f"{E.case_id(case)} r={r} pi_1={p:g}", "asym", asym, *q["asym"], worst, where)
        _, w1, _ = cpp.estimate_stress(dm, k, x2, None, 1.0)
        held(f"{E.case_id(case)} r={r}", "wsym_nokorn", w1, *q["wsym_nokorn"], worst)
    report(E.case_id(case), worst)


# --------------------------------------------------------------------------------------------------- Korn constants
def korn_handle(cpp, name, layout):
    mesh = E.mesh_of(name)
    eq = cpp.SemiExplicitEquilibrator(device_mesh(cpp, name), 2, 1, estimate_korn=True)
    if name == "disk100":                                   # the hub: both options, as include/eqlb.h asks for the Korn walk
        eq.set_option("large_patches", 1)
        eq.set_option("large_patches_stress", 1)
    eq.set_boundary(E.korn_facet_types(mesh, layout), node_mask=E.korn_node_mask(name, mesh))
    return eq


@pytest.mark.parametrize("layout", E.KORN_LAYOUTS)
@pytest.mark.parametrize("name", E.KORN_MESHES)
def test_korn_constants_against_the_oracle(cpp, oracle_mod, name, layout):
    ref, per_node, _, amp, tol = E.korn_reference(oracle_mod, name, layout)
    korn = korn_handle(cpp, name, layout).kornconst_host()
    diff = np.abs(korn - ref)
    print(f"{name} {layout}: c_K^2 in [{ref.min():.3e}, {ref.max():.3e}], largest |device - oracle| / oracle "
          f"{(diff / ref).max():.3e}, largest relative tolerance {(tol / ref).max():.3e}, "
          f"|device - oracle| / tolerance {E.ratio(diff, tol):.3f}")
    assert np.all(np.isfinite(korn)) and np.all(diff <= tol)


# ------------------------------------------------------------------------- device memory on a caller's stream, sq33
@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


class OnDevice:
    """inputs copied to device memory, outputs pre-filled with NaN, a non-default stream"""

    def __init__(self, torch):
        self.t, self.dev = torch, torch.device("cuda:0")
        self.s = torch.cuda.Stream(device=self.dev)
        self.keep = []

    def inp(self, a):
        t = self.t.from_numpy(np.array(a)).to(self.dev)                    # a copy: the data arrays are read-only
        self.keep.append(t)
        return t.data_ptr()

    def out(self, *shape):
        t = self.t.full(shape, float("nan"), dtype=self.t.float64, device=self.dev)
        self.keep.append(t)
        return t

    def run(self, call):
        self.t.cuda.synchronize()
        with self.t.cuda.stream(self.s):
            call(self.s.cuda_stream)
        self.s.synchronize()


RAW = ["estimate", "oscillation", "boundary_residual", "estimate_stress", "kornconst"]


@pytest.mark.parametrize("entry", RAW)
def test_raw_pointers_on_a_stream_equal_the_host_call(cpp, torch, entry):
    name, k, d = "sq33", 3, 2
    mesh, D, dm = E.mesh_of(name), E.data(name, k, d), device_mesh(cpp, name)
    dv = OnDevice(torch)
    x, G, f, fv, bv, korn = (dv.inp(D[n]) for n in ("x", "G", "f", "fv", "bv", "korn"))
    if entry == "estimate":
        outs = [dv.out(NRHS, mesh.ncells), dv.out(NRHS, mesh.ncells), dv.out(NRHS, mesh.nfacets)]
        dv.run(lambda s: cpp.estimate_raw(dm, k, NRHS, x, G, f, *[o.data_ptr() for o in outs], stream=s))
        ref = cpp.estimate(dm, k, D["x"], D["G"], D["f"])
    elif entry == "oscillation":
        outs = [dv.out(NRHS, mesh.ncells)]
        dv.run(lambda s: cpp.oscillation_raw(dm, k, NRHS, x, G, D["qp"], D["qw"], fv, korn, outs[0].data_ptr(), stream=s))
        ref = [cpp.oscillation(dm, k, D["x"], D["G"], D["qp"], D["qw"], D["fv"], D["korn"])]
    elif entry == "boundary_residual":
        fl = dv.inp(D["facets"])
        outs = [dv.out(NRHS, D["facets"].size)]
        dv.run(lambda s: cpp.boundary_residual_raw(dm, k, d, NRHS, x, G, D["facets"].size, fl, bv, outs[0].data_ptr(),
                                                   stream=s))
        ref = [cpp.boundary_residual(dm, k, D["x"], D["G"], D["facets"], D["bv"])]
    elif entry == "estimate_stress":
        outs = [dv.out(mesh.ncells), dv.out(mesh.ncells), dv.out(mesh.nnodes)]

        def call(s):
            st = cpp.lib().eqlb_se_estimate_stress(dm._h, C.c_int32(k), C.c_void_p(x), C.c_void_p(korn), C.c_double(50.0),
                                                   *[C.c_void_p(o.data_ptr()) for o in outs], C.c_int32(cpp.MEM_DEVICE),
                                                   C.c_void_p(s))
            assert st == 0
        dv.run(call)
        ref = cpp.estimate_stress(dm, k, D["x"][:2], D["korn"], 50.0)
    else:
        eq = korn_handle(cpp, name, "flux_left")
        outs = [dv.out(mesh.ncells)]
        outs[0].zero_()                                      # the call accumulates into its output
        torch.cuda.synchronize()

        def call(s):
            assert cpp.lib().eqlb_se_kornconst(eq._h, C.c_void_p(outs[0].data_ptr()), C.c_int32(cpp.MEM_DEVICE),
                                               C.c_void_p(s)) == 0
        dv.run(call)
        ref = [eq.kornconst_host()]
    for o, r in zip(outs, ref):
        got = o.cpu().numpy()
        assert np.all(np.isfinite(got)) and np.array_equal(got, np.asarray(r).reshape(got.shape))
