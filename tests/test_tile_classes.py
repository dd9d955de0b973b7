"""Host side of tests/test_gpu_tile_dispatch.py: the model of the tile lists (tests/tile_classes.py) on hand-counted
tiles, and the cases of the GPU file reach every body instance x bin that the tiled kernels have."""

import numpy as np

import tile_classes as tcl
import test_gpu_tile_dispatch as td


def _cnt(**kw):
    """[5, 6] class counts from keywords b<bin>c<class>=n."""
    c = np.zeros((5, 6), dtype=np.int64)
    for key, n in kw.items():
        c[int(key[1]), int(key[3])] = n
    return c


def test_flux_kernel_blocks_by_hand():
    # bin 1 (PER 8): 9 full, 7 more interior, 3 boundary = 19 patches, 3 blocks: 1 full, 1 interior (16 // 8 - 1), 1
    # generic; bin 0 (PER 16): 15 full = no whole block
    c = _cnt(b1c0=9, b1c2=7, b1c5=3, b0c0=15)
    k2 = tcl.tile_blocks(c, 2)
    assert k2["full"][:2] == [0, 1] and k2["interior"][:2] == [0, 1] and k2["generic"][:2] == [1, 1]
    k3 = tcl.tile_blocks(c, 3)    # no interior instance at k = 3
    assert k3["full"][:2] == [0, 1] and k3["interior"] == [0] * 5 and k3["generic"][:2] == [1, 2]
    k1 = tcl.tile_blocks(c, 1)    # no full instance at k = 1
    assert k1["full"] == [0] * 5 and k1["generic"][:2] == [1, 3]
    # bin 2 (PER 4): 9 interior of valence 10 - 16 -> 2 interior blocks + 1 generic at k = 2
    k2 = tcl.tile_blocks(_cnt(b2c4=9), 2)
    assert k2["interior"][2] == 2 and k2["generic"][2] == 1


def test_stress_kernel_blocks_by_hand():
    # lists of full patches: 17 full in bin 0 -> 2 blocks, 15 copies; 8 in bin 1 -> 1 block, none
    s = tcl.tile_blocks(_cnt(b0c0=17, b1c0=8, b1c5=4), 2, stress=True, mixed=False)
    assert s["full"][:2] == [2, 1] and s["padding"][:2] == [15, 0] and s["generic"] == [0] * 5
    # mixed, bin 1: full 5 | P - 1: 12 -> [5, 17): c0 1, c1 2 -> 1 block | P - 2: 7 -> [17, 24): c0 3, c1 3 -> 0 |
    # P - 3: 9 -> [24, 33): c0 3, c1 4 -> 1 block; 33 patches + 2 boundary = 35 -> 5 blocks, 0 full, 3 generic
    s = tcl.tile_blocks(_cnt(b1c0=5, b1c1=12, b1c2=7, b1c3=9, b1c5=2), 2, stress=True, mixed=True)
    assert (s["full"][1], s["nfix1"][1], s["nfix2"][1], s["nfix3"][1], s["generic"][1]) == (0, 1, 0, 1, 3)
    # bin 0 has no P - 2 / P - 3 instance (patches of 2, 1 cells): [16, 48) of valence 3 -> 2 blocks
    s = tcl.tile_blocks(_cnt(b0c0=16, b0c1=32), 2, stress=True, mixed=True)
    assert (s["full"][0], s["nfix1"][0], s["generic"][0]) == (1, 2, 0)


def test_node_classes_of_a_crossed_square():
    from dolfinx_eqlb_amd.mesh import create_unit_square
    b, c = tcl.node_bins_classes(create_unit_square(4))
    t = np.zeros((5, 6), dtype=np.int64)
    np.add.at(t, (b, c), 1)
    # 16 centres (valence 4) and 9 inner grid nodes (valence 8) are full; 12 edge nodes (5 facets), 4 corners
    assert t[0, 0] == 16 and t[1, 0] == 9 and t[1, 5] == 12 and t[0, 5] == 4 and t.sum() == 41


# every instance x bin that the tiled kernels have (flux kernel: full k >= 2, P <= 8; interior k = 2, P = 8, 16;
# fused stress kernel: bins 0, 1, NFIX where P - 1 - j >= 3)
EXPECTED = ([(("se", 1), "generic", b) for b in range(5)]
            + [((p, k), "full", b) for p in ("se", "ev", "multi") for k in (2, 3) for b in (0, 1) if (p, k) != ("multi", 3)]
            + [((p, 2), "interior", b) for p in ("se", "ev", "multi") for b in (1, 2)]
            + [(("se", k), "generic", b) for k in (2, 3) for b in range(5)]
            + [(("ev", k), "generic", b) for k in (2, 3) for b in range(3)]
            + [(("stress0", 2), kind, b) for kind in ("full", "padding") for b in (0, 1)]
            + [(("stress1", 2), kind, b) for kind, b in [("full", 0), ("full", 1), ("nfix1", 0), ("nfix1", 1),
                                                         ("nfix2", 1), ("nfix3", 1), ("generic", 0), ("generic", 1)]])


def _gpu_cases():
    """(path, k, mesh, mask) of every single-tile case of tests/test_gpu_tile_dispatch.py."""
    for name, i, counts in td.A_CASES:
        mesh = td.mesh_of(name)
        mask = td.class_mask(mesh, counts, seed=i)
        for path, k, _ in td.A_PATHS:
            yield path, k, mesh, mask
    for name in ("disk20", "disk40"):
        mesh = td.mesh_of(name)
        b, _ = tcl.node_bins_classes(mesh)
        mask = ((b >= 3) | (np.arange(mesh.nnodes) % 3 == 0)).astype(np.uint8)
        for path, k in td.LARGE_PATHS:
            yield path, k, mesh, mask
    for _, counts in td._padding_masks():
        mesh = td.mesh_of("crossed")
        yield "stress0", 2, mesh, td.class_mask(mesh, counts)


def test_gpu_cases_reach_every_instance():
    """Each GPU case asserts that tiling_blocks() equals tile_classes.predict; here: the predictions of those cases
    give every instance x bin at least one wave-block (and the padding 0 ... PER - 1 copies per bin)."""
    seen = set()
    pads = {0: set(), 1: set()}
    for path, k, mesh, mask in _gpu_cases():
        stress = path.startswith("stress")
        p = tcl.predict(mesh, k, mask, stress=stress, mixed=path == "stress1")
        for kind in tcl.KINDS:
            for b, v in enumerate(p[kind]):
                if v:
                    seen.add(((path, k), kind, b))
        if path == "stress0":
            for b in (0, 1):
                pads[b].add(p["padding"][b])
    missing = [e for e in EXPECTED if e not in seen]
    assert not missing, missing
    assert pads[0] == set(range(16)) and pads[1] == set(range(8))


def test_gpu_sweep_hits_every_residue():
    """The single-tile masks put every class of the sweep on 0, 1, PER - 1, PER, PER + 1, 2 PER - 1, 2 PER + 1."""
    for name, cls in [("crossed", [(0, 0), (1, 0)]), ("valence", [(1, 1), (1, 2)])]:
        for bc in cls:
            per = td.PER[bc[0]]
            got = {c.get(bc, 0) for n, _, c in td.A_CASES if n == name}
            assert set(td._sweep(per)) <= got, (name, bc, sorted(got))
