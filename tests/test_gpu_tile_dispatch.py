"""The tiled launches at every wave-block boundary of their tile lists, against the oracle.

k_se_patch_tiled (SE and EV, RT_1 ... RT_3), k_se_patch_tiled_multi and k_se_stress_tiled split each bin of a tile's
patch list into 64-lane wave-blocks and run a separate instance of the patch body on each kind of block (full
patches, interior patches, interior patches with P - 1, P - 2, P - 3 cells, generic; tests/tile_classes.py). The
meshes of part A and B have fewer cells than one tile, so a node mask fixes the count of every class in the tile;
the masks put those counts on the residues of PER = 64 / P where a range formula or the padding could be off by one.

Every case checks
  * tiling_blocks() (the wave-blocks each instance runs, the padding copies, the zero-flagged tiles) against the
    prediction of tests/tile_classes.py;
  * the result against the oracle over exactly the masked nodes (1e-11 relative to the largest coefficient, 1e-10
    for stress), against the slot path of the same call (scatter 0: 1e-13 at k <= 2, 1e-12 at k = 3, 1e-11 for stress),
    and bitwise against a second call of the same handle.
"""

import numpy as np
import pytest

import tile_classes as tcl

pytestmark = pytest.mark.gpu

PER = {0: 16, 1: 8, 2: 4, 3: 2, 4: 1}
START = 2.0 ** -10   # every call starts from flux_hdiv = START (below the results: the bounds stay relative to them)
FULL, P1, P2, P3, OTHER, BND = range(6)


# ---------------------------------------------------------------------------------------------------- meshes
def _refine_centroids(mesh, cells):
    """Insert the centroid of each listed cell: an interior node of 3 cells (bin 0, P - 1)."""
    from dolfinx_eqlb_amd.mesh import create_mesh
    x, cn = mesh.x[:, :2], mesh.cell_nodes
    keep = np.ones(mesh.ncells, dtype=bool)
    keep[cells] = False
    pts, new = [x], [cn[keep]]
    nid = x.shape[0]
    for c in cells:
        a, b, d = cn[c]
        pts.append(x[[a, b, d]].mean(axis=0)[None])
        new.append(np.array([[a, b, nid], [b, d, nid], [d, a, nid]]))
        nid += 1
    return create_mesh(np.concatenate(pts), np.concatenate(new))


_MESHES = {}


def mesh_of(name):
    """Single-tile meshes (fewer cells than the smallest default tile, 448 cells of the fused stress launch)."""
    if name not in _MESHES:
        from dolfinx_eqlb_amd.mesh import create_disk, create_unit_square
        from test_gpu_unstructured import delaunay_mesh
        if name == "crossed":      # full patches of bins 0 (valence 4) and 1 (valence 8), boundary patches
            m = create_unit_square(10, shuffle_seed=3, perturb=0.2)
        elif name == "valence":    # interior valence 3 (bin 0, P - 1) and 5, 6, 7 (bin 1, P - 3 ... P - 1)
            d = delaunay_mesh(130, seed=5)
            m = _refine_centroids(d, np.random.default_rng(1).choice(d.ncells, 45, replace=False))
        elif name == "fans":       # every cell split at its centroid: interior valence 10 - 16 (bin 2) and 3
            d = delaunay_mesh(40, seed=7)
            m = _refine_centroids(d, np.arange(d.ncells))
        elif name == "disk20":     # one interior patch of 20 facets (bin 3)
            m = create_disk(20, 3, shuffle_seed=2)
        elif name == "disk40":     # one interior patch of 40 facets (bin 4)
            m = create_disk(40, 2, shuffle_seed=2)
        assert m.ncells < 448, name
        _MESHES[name] = m
    return _MESHES[name]


def class_mask(mesh, counts, seed=0):
    """Node mask with counts[(bin, class)] nodes of each class (the first of a seeded permutation)."""
    b, c = tcl.node_bins_classes(mesh)
    rng = np.random.default_rng(seed)
    mask = np.zeros(mesh.nnodes, dtype=np.uint8)
    for (bi, ci), n in counts.items():
        nodes = rng.permutation(np.nonzero((b == bi) & (c == ci))[0])
        assert nodes.size >= n, (bi, ci, n, nodes.size)
        mask[nodes[:n]] = 1
    return mask


# ----------------------------------------------------------------------------------------------- references
def _oracle_se(oracle_mod, mesh, k, ft, G, f, mask, stress=False):
    ref = np.zeros((G.shape[0], mesh.ncells * k * (k + 2)))
    for node in np.nonzero(mask)[0]:
        oracle_mod.se_reconstruct(mesh, k, ft, G, f, flux_hdiv=ref, node_range=(int(node), int(node) + 1),
                                  stress=stress)
    return ref


def _oracle_ev_broken(oracle_mod, mesh, k, ft, G, f, mask):
    from dolfinx_eqlb_amd.eqlb.conforming import conforming_dofmap, conforming_to_broken
    cd, nd = conforming_dofmap(mesh, k)
    ref = np.zeros((G.shape[0], nd))
    for node in np.nonzero(mask)[0]:
        oracle_mod.ev_reconstruct(mesh, k, ft, G, f, cd, nd, flux_hdiv=ref, node_range=(int(node), int(node) + 1))
    return np.stack([conforming_to_broken(mesh, k, r) for r in ref])


def _data(mesh, k, nrhs=1, stress=False):
    """Facet types and compatible data; with nrhs > 1 the right-hand sides differ in their boundary conditions."""
    from synthetic import facet_types, make_compatible_data, make_compatible_stress_data
    if stress:
        ft = np.repeat(facet_types(mesh, None), 2, axis=0)
        G, f = make_compatible_stress_data(mesh, k, ft)
        return ft, G, f
    sides = [None, lambda p: p[:, 1] < p[:, 1].min() + 0.3 * np.ptp(p[:, 1]),
             lambda p: p[:, 0] > p[:, 0].min() + 0.5 * np.ptp(p[:, 0])]
    fts, Gs, fs = [], [], []
    for r in range(nrhs):
        ft = facet_types(mesh, sides[r % 3])
        G, f = make_compatible_data(mesh, k, ft, seed=17 + r)
        fts.append(ft[0])
        Gs.append(G)
        fs.append(f)
    return np.stack(fts), np.stack(Gs), np.stack(fs)


def _run(cpp, dm, path, k, nrhs, ft, G, f, mask, scatter=-1, accumulate=1, tile_cells=0):
    """(result of call 1, result of call 2 on the same handle, handle)."""
    if path == "ev":
        eq = cpp.ConstrainedMinEquilibrator(dm, k, nrhs)
        eq.set_option("output", 1)
    else:
        eq = cpp.SemiExplicitEquilibrator(dm, k, nrhs, reconstruct_stress=(path == "stress"))
    eq.set_option("scatter", scatter)
    if tile_cells:
        eq.set_option("tile_cells", tile_cells)
    if path == "multi":
        eq.set_option("multi_rhs", 1)
    eq.set_boundary(ft, node_mask=mask)
    eq.set_option("accumulate", accumulate)
    start = np.full((nrhs, dm.mesh.ncells * k * (k + 2)), START)
    x1 = eq.equilibrate_host(G, f, start.copy())
    x2 = eq.equilibrate_host(G, f, start.copy())
    return x1, x2, eq


def check_case(cpp, oracle_mod, monkeypatch, mesh, path, k, mask, nrhs=1, mixed=None, accumulate=1, tile_cells=0,
               tiles=None):
    """Run one case on the tiled launch; returns its tiling_blocks()."""
    stress = path == "stress"
    if stress:
        monkeypatch.setenv("EQLB_STRESS_MIXED_TILES", "1" if mixed else "0")
        k, nrhs = 2, 2
    ft, G, f = _data(mesh, k, nrhs, stress)
    dm = cpp.DeviceMesh(mesh)
    x1, x2, eq = _run(cpp, dm, path, k, nrhs, ft, G, f, mask, accumulate=accumulate, tile_cells=tile_cells)
    assert np.array_equal(x1, x2)
    if path == "ev":
        ref = _oracle_ev_broken(oracle_mod, mesh, k, ft, G, f, mask)
    else:
        ref = _oracle_se(oracle_mod, mesh, k, ft, G, f, mask, stress)
    scale = np.abs(ref).max()
    assert scale > 0.0
    ref = ref + (START if accumulate else 0.0)
    assert np.abs(x1 - ref).max() <= (1e-10 if stress else 1e-11) * scale
    xs, _, _ = _run(cpp, dm, path, k, nrhs, ft, G, f, mask, scatter=0, accumulate=accumulate)
    # (stress: the slot path has its own weak-symmetry kernel, tests/test_gpu_stress.py bounds the two at 1e-11; RT_3
    # on patches of 10 - 16 cells: the two paths round apart by 1.0e-13)
    assert np.abs(x1 - xs).max() <= (1e-11 if stress else 1e-13 if k <= 2 else 1e-12) * scale
    tb = eq.tiling_blocks()
    if tiles is not False:
        assert tb == tcl.predict(mesh, k, mask, stress, bool(mixed), tiles)
        if path != "ev":
            assert eq.tiling_info()["patch_instances"] == tcl.patch_instances(mesh, mask, stress, bool(mixed), tiles)
    return tb


# the counts each class takes: 0, 1, PER - 1, PER, PER + 1, 2 PER - 1, 2 PER + 1
def _sweep(per):
    return [0, 1, per - 1, per, per + 1, 2 * per - 1, 2 * per + 1]


def _crossed_masks():
    """Full patches of bins 0 and 1 on every residue (the two sweeps in opposite order), with boundary patches."""
    s0, s1 = _sweep(PER[0]), _sweep(PER[1])
    return [{(0, FULL): a, (1, FULL): b, (1, BND): 3, (0, BND): 1} for a, b in zip(s0, s1[::-1])]


def _valence_masks():
    """Interior patches with P - 1, P - 2, P - 3 cells behind the class before them: ranges that start and end
    inside one wave-block, that are empty (c1 < c0) and that are exactly one block; bin 0: valence 3 behind the
    full valence-4 patches."""
    out = []
    for a, b in zip(_sweep(PER[1]), _sweep(PER[1])[::-1]):   # P - 1 (7 cells) and P - 2 (6 cells) of bin 1
        out.append({(1, P1): a, (1, P2): b, (1, P3): 3, (1, BND): 2, (0, BND): 2})
    # (full, P - 1, P - 2, P - 3) of bin 1 and (full, P - 1) of bin 0: [3, 7) inside block 0 (c1 < c0), [8, 16) one
    # block, [5, 17) from inside block 0 to inside block 2, a range right behind a partial one
    for nf, n1, n2, n3, f0, v0 in [(3, 4, 9, 8, 3, 12), (8, 8, 0, 8, 0, 16), (5, 12, 7, 1, 9, 23),
                                   (15, 1, 15, 17, 5, 11), (0, 17, 16, 15, 1, 33)]:
        out.append({(1, FULL): nf, (1, P1): n1, (1, P2): n2, (1, P3): n3, (0, FULL): f0, (0, P1): v0,
                    (1, BND): 1, (0, BND): 1})
    return out


def _fan_masks():
    """Interior patches of bin 2 (valence 10 - 16; the interior instance at k = 2, PER = 4): 0, 1, 3, 4, 5, 7, 9."""
    return [{(2, OTHER): a, (2, P2): b, (2, BND): 1, (0, P1): 3} for a, b in [(0, 0), (1, 0), (3, 0), (4, 0), (3, 2),
                                                                             (7, 0), (7, 2)]]


A_CASES = ([("crossed", i, m) for i, m in enumerate(_crossed_masks())]
           + [("valence", i, m) for i, m in enumerate(_valence_masks())]
           + [("fans", i, m) for i, m in enumerate(_fan_masks())])
A_PATHS = [("se", 1, 1), ("se", 2, 1), ("se", 3, 1), ("ev", 2, 1), ("ev", 3, 1), ("multi", 2, 2), ("multi", 2, 3),
           ("stress0", 2, 2), ("stress1", 2, 2)]


@pytest.fixture(scope="module")
def cpp():
    from dolfinx_eqlb_amd import cpp as c
    assert c.device_count() >= 1, "GPU tests need a HIP device"
    return c


@pytest.mark.parametrize("path,k,nrhs", A_PATHS, ids=[f"{p}-k{k}-r{r}" for p, k, r in A_PATHS])
@pytest.mark.parametrize("mesh_name,i,counts", A_CASES, ids=[f"{n}{i}" for n, i, _ in A_CASES])
def test_single_tile_class_sweep(cpp, oracle_mod, monkeypatch, mesh_name, i, counts, path, k, nrhs):
    """Part A: one tile, every class count on the residues of PER that bound a wave-block range."""
    mesh = mesh_of(mesh_name)
    mask = class_mask(mesh, counts, seed=i)
    name = "stress" if path.startswith("stress") else path
    check_case(cpp, oracle_mod, monkeypatch, mesh, name, k, mask, nrhs=nrhs, mixed=path == "stress1")


LARGE_PATHS = [("se", 1), ("se", 2), ("se", 3), ("ev", 2), ("stress1", 2)]


@pytest.mark.parametrize("path,k", LARGE_PATHS)
@pytest.mark.parametrize("mesh_name", ["disk20", "disk40"])
def test_single_tile_large_patches(cpp, oracle_mod, monkeypatch, mesh_name, path, k):
    """Bins 3 and 4 (patches of 17 - 32 and 33 - 64 facets): the generic body of the flux kernel; the fused stress
    launch leaves them to the generic kernels."""
    mesh = mesh_of(mesh_name)
    b, c = tcl.node_bins_classes(mesh)
    mask = ((b >= 3) | (np.arange(mesh.nnodes) % 3 == 0)).astype(np.uint8)
    name = "stress" if path.startswith("stress") else path
    check_case(cpp, oracle_mod, monkeypatch, mesh, name, k, mask, mixed=True)


def _padding_masks():
    """Fused stress launch with lists of full patches only: bin 0 on all 16 residues (0 ... 15 padding copies),
    bin 1 on all 8; one bin empty and the other not; no rest (full patches only), a rest without full patches."""
    out = []
    for n in range(1, 17):
        out.append(("res%d" % n, {(0, FULL): n, (1, FULL): (n - 1) % 8 + 1 + 8 * (n > 8), (1, BND): n % 3}))
    out += [("bin0-empty", {(1, FULL): 5, (1, BND): 2}), ("bin1-empty", {(0, FULL): 7, (0, BND): 1}),
            ("no-rest", {(0, FULL): 17, (1, FULL): 9}), ("rest-only", {(1, BND): 6, (0, BND): 2}),
            ("bin0-empty-no-rest", {(1, FULL): 8}), ("bin1-empty-no-rest", {(0, FULL): 1})]
    return out


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("name,counts", _padding_masks(), ids=[n for n, _ in _padding_masks()])
def test_fused_stress_padding_and_rest(cpp, oracle_mod, monkeypatch, name, counts, accumulate):
    """Part B: the padding copies of the lists of full patches (k_se_stress_tiled<false>) and the rest that the
    generic kernels add behind it, with += and = semantics, twice on the same handle."""
    mesh = mesh_of("crossed")
    mask = class_mask(mesh, counts)
    tb = check_case(cpp, oracle_mod, monkeypatch, mesh, "stress", 2, mask, mixed=False, accumulate=accumulate)
    nf = [counts.get((b, FULL), 0) for b in (0, 1)]
    assert tb["padding"][:2] == [(-n) % PER[b] for b, n in enumerate(nf)]


def _small_tiles_meshes():
    from dolfinx_eqlb_amd.mesh import create_unit_square
    from test_gpu_unstructured import delaunay_mesh
    return {"crossed20": create_unit_square(20, shuffle_seed=11, perturb=0.2), "delaunay1500": delaunay_mesh(1500, 3)}


@pytest.fixture(scope="module")
def small_tile_meshes():
    return _small_tiles_meshes()


@pytest.mark.parametrize("path,k", [("se", 2), ("se", 3), ("ev", 2), ("stress0", 2), ("stress1", 2)])
@pytest.mark.parametrize("tile_cells", [1, 2, 3, 7, 31, 64, 0])
@pytest.mark.parametrize("mesh_name", ["crossed20", "delaunay1500"])
def test_many_small_tiles(cpp, oracle_mod, monkeypatch, small_tile_meshes, mesh_name, tile_cells, path, k):
    """Part C: many tiles (option tile_cells; 0 = the default), unmasked and on half of the domain."""
    mesh = small_tile_meshes[mesh_name]
    name = "stress" if path.startswith("stress") else path
    for half in (False, True):
        mask = (mesh.x[:, 0] < np.median(mesh.x[:, 0])).astype(np.uint8) if half else np.ones(mesh.nnodes, np.uint8)
        tiles = [np.array([c]) for c in range(mesh.ncells)] if tile_cells == 1 else False
        tb = check_case(cpp, oracle_mod, monkeypatch, mesh, name, k, mask, mixed=path == "stress1",
                        tile_cells=tile_cells, tiles=tiles)
        if tile_cells == 1 and name == "se" and not half:
            dm = cpp.DeviceMesh(mesh)
            eq = cpp.SemiExplicitEquilibrator(dm, k, 1)
            eq.set_option("tile_cells", 1)
            eq.set_boundary(_data(mesh, k)[0])
            info = eq.tiling_info()
            assert info["ntiles"] == mesh.ncells and info["patch_instances"] == 3 * mesh.ncells
        if half:
            assert tb["zero_tiles"] > 0
