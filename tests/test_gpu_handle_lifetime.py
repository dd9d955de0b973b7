"""What the mesh and equilibrator handles own, seen from outside: the first use of the node -> cell table, alone and from
two host threads at once, the wrap of the ring of timing events, and handles that are created, used once and closed
over and over.  Everything is compared bit for bit with the same call on a handle in a known state; no magnitude is
asserted.

The mesh is the 4 x 4 crossed unit square (4 triangles per square: 64 cells), uploaded with cpp.DeviceMesh(mesh): the
eqlb_mesh_create route, where node_cells stays on the host until a consumer asks for it.  The four consumers are
export() with node_cells, estimate_stress at RT_2, PrimalPoisson(dm, 2) + diagonal(), and Refinement.prolong at p = 2
after marking two cells.  The prolongation reads node_cells of the REFINED mesh, and the refined handle that
DeviceMesh.refine returns is built on the device with the table in place; so the prolongation - and every pairing it
takes part in - runs on a fresh cpp.DeviceMesh of the refined mesh's host tables, with the plan of the refinement kept.

The ring wrap is asserted here: tests/test_gpu_kernel_timing.py records two calls per handle and never reaches the
64 sets of the ring."""

import itertools
import math
import threading

import numpy as np
import pytest

from dolfinx_eqlb_amd.mesh import create_unit_square
from synthetic import facet_types, make_compatible_data, make_compatible_stress_data

pytestmark = pytest.mark.gpu

K, P = 2, 2
NRT = K * (K + 2)


class Ctx:
    """The two host meshes, the kept plan between them and the input data; the consumers only read them."""

    def __init__(self):
        from dolfinx_eqlb_amd import cpp
        assert cpp.device_count() >= 1, "GPU tests need a HIP device"
        self.cpp = cpp
        rng = np.random.default_rng(20261019)
        self.square = create_unit_square(4)
        assert self.square.ncells == 64
        self.coarse = cpp.DeviceMesh(self.square)
        self.ref = self.coarse.refine(np.array([0, 5], dtype=np.int32), keep_plan=True)
        self.fine = self.ref.dmesh.mesh
        assert self.ref.counts["nbisected"] > 0 and self.fine.ncells > self.square.ncells
        self.meshes = {"square": self.square, "fine": self.fine}
        self.x = {kind: rng.standard_normal((2, m.ncells * NRT)) for kind, m in self.meshes.items()}
        self.korn = {kind: 1.0 + rng.random(m.ncells) for kind, m in self.meshes.items()}
        self.u = rng.standard_normal(self.coarse.lagrange_dofmap(P)[1])
        self._expected = {}

    def fresh(self, kind):
        """A handle of eqlb_mesh_create on which nothing has asked for node_cells yet."""
        return self.cpp.DeviceMesh(self.meshes[kind])

    def expected(self, kind, consumer):
        """The consumer's result on a handle where export() ran first, computed once per mesh."""
        if (kind, consumer) not in self._expected:
            dm = self.fresh(kind)
            dm.export()
            self._expected[kind, consumer] = consumer(self, kind, dm)
            dm.close()
        return self._expected[kind, consumer]

    def close(self):
        self.ref.close()
        self.ref.dmesh.close()
        self.coarse.close()


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


# ---- the four consumers of node_cells: (ctx, kind of mesh, handle) -> list of result arrays ------------------------
def export(c, kind, dm):
    t = dm.export()
    assert np.array_equal(t["node_cells"], c.meshes[kind].node_cells)
    return [t[name] for name in sorted(t)]


def estimate_stress(c, kind, dm):
    return list(c.cpp.estimate_stress(dm, K, c.x[kind], korn=c.korn[kind], pi_1=1.5))


def primal_diagonal(c, kind, dm):
    op = c.cpp.PrimalPoisson(dm, P)
    out = op.diagonal()
    op.close()
    return [out]


def prolong(c, kind, dm):
    assert kind == "fine"
    r = c.ref
    return [c.cpp.Refinement(dm, r.parent_cell, r.node_parent_facet, r.parent_facet, r.counts, r.plan).prolong(P, c.u)]


CONSUMERS = [export, estimate_stress, primal_diagonal, prolong]


def _kind(*consumers):
    return "fine" if prolong in consumers else "square"


def _same(got, want, who):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        if a.dtype.kind == "f":
            assert np.isfinite(a).all() and np.count_nonzero(a) > 0, (who, i)
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (who, i)


@pytest.mark.parametrize("consumer", CONSUMERS, ids=[f.__name__ for f in CONSUMERS])
def test_first_use_of_node_cells(ctx, consumer):
    kind = _kind(consumer)
    want = ctx.expected(kind, consumer)
    dm = ctx.fresh(kind)
    got = consumer(ctx, kind, dm)
    dm.close()
    _same(got, want, consumer.__name__)


@pytest.mark.parametrize("pair", list(itertools.combinations(CONSUMERS, 2)),
                         ids=lambda p: "-".join(f.__name__ for f in p))
def test_first_use_from_two_threads(ctx, pair):
    """Both threads leave the barrier together and meet a handle without node_cells; ctypes releases the GIL for the
    length of every call into the library.  One run per pairing."""
    kind = _kind(*pair)
    want = [ctx.expected(kind, f) for f in pair]
    dm = ctx.fresh(kind)
    barrier = threading.Barrier(2)
    got, errors = [None, None], []

    def run(i):
        try:
            barrier.wait()
            got[i] = pair[i](ctx, kind, dm)
        except BaseException as e:  # (reported by the main thread)
            errors.append((pair[i].__name__, repr(e)))

    threads = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    dm.close()
    assert not errors, errors
    for f, g, w in zip(pair, got, want):
        _same(g, w, f.__name__)


def test_timing_ring_wraps(ctx):
    """70 timed calls on a ring of 64 event sets: the sets of the first six calls are recorded a second time."""
    cpp, mesh = ctx.cpp, ctx.square
    ft = facet_types(mesh)
    G, f = make_compatible_data(mesh, K, ft)
    dm = cpp.DeviceMesh(mesh)
    eq = cpp.SemiExplicitEquilibrator(dm, K, 1)
    eq.set_option("timing", 1)
    eq.set_boundary(ft)
    first = eq.equilibrate_host(G[None], f[None])
    for _ in range(68):
        eq.equilibrate_host(G[None], f[None])
    last = eq.equilibrate_host(G[None], f[None])
    ms = eq.last_kernel_ms(0)
    eq.check_status()
    eq.close()
    dm.close()
    print("last_kernel_ms(0) after 70 calls:", ms)
    assert math.isfinite(ms) and ms > 0.0
    assert np.count_nonzero(first) > 0 and first.tobytes() == last.tobytes()


def test_create_use_and_drop_twenty_times(ctx, monkeypatch):
    """A stress handle (two rows at RT_2: the fused launch) and an EV handle, each created, used once and closed, 20
    times in one process.  On a mesh this small more than 5 % of the patches are not full, and the tiles would list
    them all: EQLB_STRESS_MIXED_TILES=0 keeps the tile lists to the full patches, so the 16 boundary patches are the
    REST, which the sweep runs on the side lane of the handle - created, used and destroyed in every cycle."""
    cpp, mesh = ctx.cpp, ctx.square
    monkeypatch.setenv("EQLB_STRESS_MIXED_TILES", "0")  # (read by every set_boundary)
    ft = facet_types(mesh)
    ft2 = np.repeat(facet_types(mesh, None), 2, axis=0)
    G, f = make_compatible_data(mesh, K, ft)
    G2, f2 = make_compatible_stress_data(mesh, K, ft2)
    nc, nf = np.diff(mesh.node_cells_offsets), np.diff(mesh.node_facets_offsets)
    nfull = int(np.count_nonzero((nc == nf) & ((nc == 4) | (nc == 8))))
    assert nf.max() <= 8 and 0 < nfull < mesh.nnodes  # one bin pair, and patches that are not full
    dm = cpp.DeviceMesh(mesh)
    want = None
    for _ in range(20):
        stress = cpp.SemiExplicitEquilibrator(dm, K, 2, reconstruct_stress=True)
        stress.set_boundary(ft2)
        # a rest exists: the tiles hold wave-blocks of full patches (and their padding) only, fewer than all patches
        blocks, info = stress.tiling_blocks(), stress.tiling_info()
        assert info["ntiles"] >= 1 and sum(blocks["full"]) > 0
        assert all(sum(blocks[kind]) == 0 for kind in ("interior", "nfix1", "nfix2", "nfix3", "generic"))
        assert stress.num_patches - nfull == 16
        ev = cpp.ConstrainedMinEquilibrator(dm, K, 1)
        ev.set_boundary(ft)
        got = (stress.equilibrate_host(G2, f2), ev.equilibrate_host(G[None], f[None]))
        stress.check_status()
        ev.check_status()
        stress.close()
        ev.close()
        if want is None:
            print("tiling_info:", info, "tiling_blocks:", blocks)
            want = got
            assert all(np.isfinite(a).all() and np.count_nonzero(a) > 0 for a in want)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    dm.close()
