"""Python model of the tile lists of the tiled launches (test helper).

Restates how the tile builder classifies and orders the nodes of a tile, and how the tiled kernels split each
bin of the list into 64-lane wave-blocks, to predict eqlb_se_tiling_blocks exactly:

  * bin b of a node: the smallest P in (4, 8, 16, 32, 64) with P >= its number of facets;
  * class: 0 full (interior, P cells) | 1, 2, 3 interior with P - 1, P - 2, P - 3 cells | 4 other interior |
    5 boundary (a boundary facet at the node); a tile lists its nodes by (bin, class);
  * PER = 64 / P patches per wave-block; block u of a bin holds the patches [u PER, (u + 1) PER).

Flux kernel (k_se_patch_tiled*): the whole blocks of full patches run the full-patch body (k >= 2, P <= 8),
the whole blocks of interior patches behind them the interior body (k = 2, P = 8, 16), the rest the generic body.
Fused stress kernel (k_se_stress_tiled, bins 0, 1): with lists of full patches only (mixed = False) every
block runs the full-patch body and the lists are padded to whole blocks with copies; with mixed lists the whole
blocks inside the ranges of interior patches with P - 1, P - 2, P - 3 (>= 3) cells run their own instances.
"""

import numpy as np

PS = (4, 8, 16, 32, 64)
KINDS = ("full", "interior", "nfix1", "nfix2", "nfix3", "generic", "padding")
NCLASS = 6


def node_bins_classes(mesh):
    """(bin, class) of every node."""
    ncells = np.diff(mesh.node_cells_offsets)
    nfcts = np.diff(mesh.node_facets_offsets)
    b = np.searchsorted(np.array(PS), nfcts, side="left")
    P = np.array(PS)[np.minimum(b, len(PS) - 1)]
    interior = ncells == nfcts
    missing = P - ncells
    cls = np.where(interior, np.where((missing >= 0) & (missing <= 3), missing, 4), 5)
    return b.astype(np.int64), cls.astype(np.int64)


def _listed(mesh, node_mask, stress, mixed):
    """Nodes the tiles list: masked in; for the fused stress launch bins 0, 1 only, and full patches only
    without mixed lists (the others go to the generic kernels)."""
    b, cls = node_bins_classes(mesh)
    listed = np.ones(mesh.nnodes, dtype=bool) if node_mask is None else np.asarray(node_mask).astype(bool)
    if stress:
        listed &= b < 2
        if not mixed:
            listed &= cls == 0
    return listed, b, cls


def tile_class_counts(mesh, cells, node_mask=None, stress=False, mixed=False):
    """[5, 6] counts (bin, class) of the listed nodes of the tile made of `cells`, and its zero flag."""
    listed, b, cls = _listed(mesh, node_mask, stress, mixed)
    nodes = np.unique(mesh.cell_nodes[np.asarray(cells)].ravel())
    zero = bool((~listed[nodes]).any())
    nodes = nodes[listed[nodes]]
    cnt = np.zeros((len(PS), NCLASS), dtype=np.int64)
    np.add.at(cnt, (b[nodes], cls[nodes]), 1)
    return cnt, zero


def tile_blocks(cnt, k, stress=False, mixed=False):
    """dict kind -> [count per bin] of ONE tile with class counts cnt [5, 6]."""
    out = {kind: [0] * len(PS) for kind in KINDS}
    for bi, P in enumerate(PS):
        per = 64 // P
        c = [int(v) for v in cnt[bi]]
        nfull, nint, np_ = c[0], sum(c[:5]), sum(c)
        if stress:
            if bi >= 2:
                continue
            if not mixed:
                padded = -(-nfull // per) * per
                out["full"][bi] += padded // per
                out["padding"][bi] += padded - nfull
                continue
            nwb = -(-np_ // per)
            nwb_full = nfull // per
            ends = [nfull + sum(c[1:j + 2]) for j in range(3)]   # nval: end of the class with P - 1 - j cells
            starts = [nfull] + ends[:2]
            nfix = 0
            for j in range(3):
                if P - 1 - j >= 3:
                    c0, c1 = -(-starts[j] // per), ends[j] // per
                    n = max(c1 - c0, 0)
                    out[f"nfix{j + 1}"][bi] += n
                    nfix += n
            out["full"][bi] += nwb_full
            out["generic"][bi] += nwb - nwb_full - nfix
            continue
        nwb = -(-np_ // per)
        nwb_full = nfull // per if (k >= 2 and P <= 8) else 0
        nwb_int = nint // per if (k == 2 and P in (8, 16)) else 0
        ni = max(nwb_int - nwb_full, 0)
        out["full"][bi] += nwb_full
        out["interior"][bi] += ni
        out["generic"][bi] += nwb - nwb_full - ni
    return out


def predict(mesh, k, node_mask=None, stress=False, mixed=False, tiles=None):
    """The expected tiling_blocks() of a handle: `tiles` lists the cells of each tile (default: the whole mesh is
    one tile, i.e. it has fewer cells than a tile)."""
    if tiles is None:
        tiles = [np.arange(mesh.ncells)]
    total = {kind: [0] * len(PS) for kind in KINDS}
    total["zero_tiles"] = 0
    for cells in tiles:
        cnt, zero = tile_class_counts(mesh, cells, node_mask, stress, mixed)
        for kind, v in tile_blocks(cnt, k, stress, mixed).items():
            total[kind] = [a + b for a, b in zip(total[kind], v)]
        total["zero_tiles"] += int(zero)
    return total


def patch_instances(mesh, node_mask=None, stress=False, mixed=False, tiles=None):
    """Patch instances of the tiling (padding copies included)."""
    if tiles is None:
        tiles = [np.arange(mesh.ncells)]
    n = 0
    for cells in tiles:
        cnt, _ = tile_class_counts(mesh, cells, node_mask, stress, mixed)
        if stress and not mixed:
            n += sum(-(-int(cnt[bi, 0]) // (64 // PS[bi])) * (64 // PS[bi]) for bi in range(2))
        else:
            n += int(cnt.sum())
    return n
