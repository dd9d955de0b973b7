"""Full 8-cell patches of RT_2 in the tiled flux sweep, at every boundary of the split of their list.

A tile lists its full 8-cell patches first (TileDesc::nfull). With EQLB_PAIR_LANES (eqlb_se_kernels_pair.hip) the
whole wave-blocks of 16 of them run four lanes per patch, two ring cells per lane, the remainder of fewer than 16 runs
the full-patch instance, 8 per wave-block, and what is left after that the generic instance; without the switch the
same lists run 8 per wave-block throughout. The cases put the number of full 8-cell patches of a tile on 0, 1, 15, 16,
17 and 33, so every piece of the split is empty, partial and whole once, on a mesh with shuffled local vertex order
(reversed facets, det J < 0) and with a node mask that leaves rows of owned cells unwritten; they hold for either
value of the switch.

Bounds: against the oracle the one of the tiled-vs-oracle tests (tests/test_gpu_parity.py: RTOL = 1e-11 relative to
the largest coefficient), two runs of the same call bitwise equal; check_case (tests/test_gpu_tile_dispatch.py) adds
the slot path of the same call at 1e-13 and the prediction of tiling_blocks().
"""

import numpy as np
import pytest

import tile_classes as tcl
from cases import make_case
from test_gpu_parity import RTOL
from test_gpu_tile_dispatch import BND, FULL, check_case, class_mask, mesh_of

pytestmark = pytest.mark.gpu

NFULL8 = [0, 1, 15, 16, 17, 33]


@pytest.fixture(scope="module")
def cpp():
    from dolfinx_eqlb_amd import cpp as c
    assert c.device_count() >= 1, "GPU tests need a HIP device"
    return c


def split_of(nfull):
    """(wave-blocks of 16 patches, 64-lane wave-blocks of 8 behind them, full patches left to the generic instance)."""
    return nfull // 16, (nfull % 16) // 8, nfull % 8


def test_split_model():
    assert [split_of(n) for n in NFULL8] == [(0, 0, 0), (0, 0, 1), (0, 1, 7), (1, 0, 0), (1, 0, 1), (2, 0, 1)]


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("nfull", NFULL8)
def test_full_patch_counts(cpp, oracle_mod, monkeypatch, nfull, accumulate):
    """One tile (the 10 x 10 crossed mesh: 400 cells, 81 full 8-cell patches) whose node mask leaves `nfull` of them,
    with full 4-cell patches and boundary patches of both bins behind them."""
    mesh = mesh_of("crossed")
    mask = class_mask(mesh, {(1, FULL): nfull, (0, FULL): 5, (1, BND): 3, (0, BND): 1}, seed=nfull)
    cnt, zero = tcl.tile_class_counts(mesh, np.arange(mesh.ncells), mask)
    assert cnt[1, FULL] == nfull and cnt[0, FULL] == 5 and zero   # (masked-out vertices: rows never written)
    tb = check_case(cpp, oracle_mod, monkeypatch, mesh, "se", 2, mask, accumulate=accumulate)
    # 64-lane blocks of full patches of the bin P = 8: two per wave-block of 16 patches, one for a remainder of 8 - 15
    npair, nrest, _ = split_of(nfull)
    assert tb["full"][1] == 2 * npair + nrest == nfull // 8
    assert tb["zero_tiles"] == 1


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("bc", ["dirichlet", "neumann_lt"])
def test_crossed_20(cpp, oracle_mod, bc, accumulate):
    """The 20 x 20 crossed mesh of test_tiled_scatter_is_bitwise_the_slot_path: several tiles with rims, 361 full
    8-cell patches spread over them."""
    mesh, ft, G, f = make_case(20, 2, bc)
    dm = cpp.DeviceMesh(mesh)
    eq = cpp.SemiExplicitEquilibrator(dm, 2, 1)
    eq.set_option("scatter", 2)
    eq.set_boundary(ft)
    eq.set_option("accumulate", accumulate)
    tb = eq.tiling_blocks()
    assert tb["full"][1] >= 2 * eq.tiling_info()["ntiles"]   # every tile has at least one wave-block of 16 full patches
    start = np.full((1, mesh.ncells * 8), 2.0 ** -10)
    x1 = eq.equilibrate_host(G, f, start.copy())
    x2 = eq.equilibrate_host(G, f, start.copy())
    assert np.array_equal(x1, x2)
    ref = oracle_mod.se_reconstruct(mesh, 2, ft, G, f)
    scale = np.abs(ref).max()
    err = np.abs(x1 - (ref + (2.0 ** -10 if accumulate else 0.0))).max()
    print(f"crossed 20 x 20, {bc}, accumulate {accumulate}: {err / scale:.3e} of the largest coefficient")
    assert err <= RTOL * scale
