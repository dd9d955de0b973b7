"""Timing slots of the equilibration sweep (option "timing", eqlb_se_last_kernel_ms): which of the slots
which = 0 ... 7 (0 - 4 patch kernel of the bin P = 4 << which, 5 reduction, 6 weak symmetry, 7 large-patch kernel) hold
a time after two calls, and which read exactly 0.0, on every route through the sweep.  No magnitude is asserted.

The expected pattern of a route follows from where the sweep records events and from what the getter reports:
  * a launch of all bins at once (slot or atomic scatter with "fused", EV at k <= 3, every tiled launch) is timed in
    slot 0, the slots 1 - 4 read 0.0; launches per bin are timed in the slot of their bin, and a bin without patches
    reads 0.0 (bin of a patch: the smallest P of 4, 8, 16, 32, 64 that holds its facets);
  * slot 5 holds the reduction of the slot scatter (EV: the reduction to the conforming DOFs) and reads 0.0 on the
    tiled and the atomic route;
  * slot 6 holds the weak-symmetry kernels of the slot path of a stress handle; the fused stress launch has no kernel
    of its own for them, and the rest it leaves to the generic kernels runs untimed next to it: 0.0;
  * slot 7 holds the large-patch kernel of a handle with "large_patches", on the slot and on the tiled route."""

import functools

import numpy as np
import pytest

from dolfinx_eqlb_amd.mesh import create_disk, create_unit_square
from synthetic import facet_types, make_compatible_data, make_compatible_stress_data
from test_large_patches_oracle import disk_case

pytestmark = pytest.mark.gpu

SLOTS, ATOMIC, TILED = 0, 1, 2
ALL_BINS_IN_ONE = (0,)


@pytest.fixture(scope="module")
def cpp():
    from dolfinx_eqlb_amd import cpp as c
    assert c.device_count() >= 1, "GPU tests need a HIP device"
    return c


@pytest.fixture(autouse=True)
def _clear_hip_last_error():
    """Reading a slot whose events were never recorded (slot 6 of a fused stress launch) ends in a failing
    hipEventElapsedTime inside the getter; the getter answers 0.0, but the runtime keeps the error as the thread's last
    one, and the next kernel launch of the library would report it.  Later tests start clean."""
    yield
    import ctypes
    for name in (None, "libamdhip64.so"):
        try:
            ctypes.CDLL(name).hipGetLastError()
            return
        except (AttributeError, OSError):
            continue


@functools.lru_cache(maxsize=None)
def _square(k):
    mesh = create_unit_square(8)
    ft = facet_types(mesh)
    G, f = make_compatible_data(mesh, k, ft)
    return mesh, ft, G[None], f[None]


@functools.lru_cache(maxsize=None)
def _stress(kind, k):
    mesh = create_unit_square(8) if kind == "square" else create_disk(12, 3, shuffle_seed=9)
    ft = np.repeat(facet_types(mesh, None), 2, axis=0)
    G, f = make_compatible_stress_data(mesh, k, ft)
    return mesh, ft, G, f


def _bins(mesh, skip_large=False):
    """Bins that hold a patch: P = 4 << b is the smallest that takes the facets of the patch."""
    out = set()
    for nf, nc in zip(np.diff(mesh.node_facets_offsets), np.diff(mesh.node_cells_offsets)):
        if skip_large and (nf > 64 or nc > 63):
            continue
        out.add(next(b for b in range(5) if (4 << b) >= nf))
    return tuple(sorted(out))


def _pattern(eq, G, f):
    eq.set_option("timing", 1)
    for _ in range(2):
        eq.equilibrate_host(G, f)
    ms = [eq.last_kernel_ms(w) for w in range(8)]
    print("last_kernel_ms:", ms)
    assert all(t >= 0.0 for t in ms)
    return tuple(w for w in range(8) if ms[w] != 0.0)


def _se(cpp, mesh, ft, k, nrhs=1, stress=False, **opts):
    eq = cpp.SemiExplicitEquilibrator(cpp.DeviceMesh(mesh), k, nrhs, reconstruct_stress=stress)
    for key, v in opts.items():
        eq.set_option(key, v)
    eq.set_boundary(ft)
    return eq


def test_bins_of_the_square():
    """The crossed square has patches in the bins 0 and 1 only (the per-bin cases below rest on it)."""
    assert _bins(_square(2)[0]) == (0, 1)


def test_slots_per_bin(cpp):
    mesh, ft, G, f = _square(2)
    eq = _se(cpp, mesh, ft, 2, scatter=SLOTS, fused=0)
    assert _pattern(eq, G, f) == _bins(mesh) + (5,)


def test_slots_fused(cpp):
    mesh, ft, G, f = _square(2)
    eq = _se(cpp, mesh, ft, 2, scatter=SLOTS)
    assert _pattern(eq, G, f) == ALL_BINS_IN_ONE + (5,)


@pytest.mark.parametrize("scatter", [TILED, -1], ids=["tiled", "auto"])
def test_tiled(cpp, scatter):
    mesh, ft, G, f = _square(2)
    eq = _se(cpp, mesh, ft, 2, scatter=scatter)
    assert _pattern(eq, G, f) == ALL_BINS_IN_ONE


@pytest.mark.parametrize("fused", [1, 0])
def test_atomic(cpp, fused):
    mesh, ft, G, f = _square(2)
    eq = _se(cpp, mesh, ft, 2, scatter=ATOMIC, fused=fused)
    assert _pattern(eq, G, f) == (ALL_BINS_IN_ONE if fused else _bins(mesh))


@pytest.mark.parametrize("scatter", [SLOTS, TILED], ids=["slots", "tiled"])
def test_ev(cpp, scatter):
    mesh, ft, G, f = _square(2)
    eq = cpp.ConstrainedMinEquilibrator(cpp.DeviceMesh(mesh), 2, 1)
    eq.set_option("scatter", scatter)
    eq.set_boundary(ft)
    assert _pattern(eq, G, f) == ALL_BINS_IN_ONE + ((5,) if scatter == SLOTS else ())


@pytest.mark.parametrize("fused", [1, 0])
def test_stress_on_the_slot_path(cpp, fused):
    """RT_3: no fused stress launch, the automatic scatter resolves to the slots."""
    mesh, ft, G, f = _stress("square", 3)
    eq = _se(cpp, mesh, ft, 3, nrhs=2, stress=True, fused=fused)
    assert _pattern(eq, G, f) == (ALL_BINS_IN_ONE if fused else _bins(mesh)) + (5, 6)


@pytest.mark.parametrize("kind", ["square", "disk"])
def test_fused_stress(cpp, kind):
    """RT_2 without flux BCs on the stress rows: one tiled launch.  On the disk the hub (12 cells, bin 2) is left to
    the generic kernels: patch and weak-symmetry kernels on the side stream, compact reduction - all untimed."""
    mesh, ft, G, f = _stress(kind, 2)
    assert (2 in _bins(mesh)) == (kind == "disk")
    eq = _se(cpp, mesh, ft, 2, nrhs=2, stress=True)
    assert _pattern(eq, G, f) == ALL_BINS_IN_ONE


@pytest.mark.parametrize("scatter,fused", [(SLOTS, 1), (SLOTS, 0), (TILED, 1)],
                         ids=["slots", "slots-per-bin", "tiled"])
def test_large_patches(cpp, scatter, fused):
    """Disk whose hub has 64 cells: the large-patch kernel is timed in slot 7 on both routes."""
    mesh, ft, G, f = disk_case(64, 2, 2)
    eq = cpp.SemiExplicitEquilibrator(cpp.DeviceMesh(mesh), 2, 1)
    eq.set_option("scatter", scatter)
    eq.set_option("fused", fused)
    eq.set_option("large_patches", 1)
    eq.set_boundary(ft)
    assert eq.large_patch_info() == (1, 64)
    bins = ALL_BINS_IN_ONE if (fused or scatter == TILED) else _bins(mesh, skip_large=True)
    assert _pattern(eq, G, f) == bins + ((5,) if scatter == SLOTS else ()) + (7,)


def test_timing_off_reads_zero(cpp):
    mesh, ft, G, f = _square(2)
    eq = _se(cpp, mesh, ft, 2)
    eq.equilibrate_host(G, f)
    assert [eq.last_kernel_ms(w) for w in range(8)] == [0.0] * 8
