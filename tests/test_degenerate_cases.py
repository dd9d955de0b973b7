"""The meshes of tests/degenerate_cases.py on the host (no GPU): what tests/test_gpu_degenerate_cells.py relies on.

  * det J of the bad cell is exactly 0.0 in the expression the kernels use, in every local vertex order, and no other
    cell is flat; the counts and valences are the documented ones;
  * the oracle over node_range of every node that is not a vertex of the bad cell is finite (that sum is the
    reference of the GPU tests), the unrestricted oracle refuses the mesh with status -2;
  * the (bin, class) of the bad cell's vertices in the tile lists, which decides the instances the GPU cases reach."""

import itertools

import numpy as np
import pytest

import degenerate_cases as dc

NAMES = sorted(dc.BUILDERS)


@pytest.mark.parametrize("name", NAMES)
def test_bad_cell_is_exactly_flat(name):
    mesh, bad = dc.case(name)       # (asserts det == 0.0, the cell counts and the valences of dc.EXPECT)
    ncells, nfar, val = dc.EXPECT[name]
    assert (mesh.ncells, dc.far_cells(mesh, bad).size, dc.valences(mesh, bad)) == (ncells, nfar, val)
    assert mesh.ncells <= 260
    # every local vertex order, with and without a fused multiply-add in J00 J11 - J01 J10
    x = mesh.x[mesh.cell_nodes[bad], :2]
    for p in itertools.permutations(range(3)):
        J = np.stack([x[p[1]] - x[p[0]], x[p[2]] - x[p[0]]], axis=1)
        assert J[0, 0] * J[1, 1] - J[0, 1] * J[1, 0] == 0.0
        # exact products: each one is representable, so an fma sees the same two numbers
        for a, b in ((J[0, 0], J[1, 1]), (J[0, 1], J[1, 0])):
            assert float(np.longdouble(a) * np.longdouble(b)) == a * b and (a * b == 0.0 or abs(a * b) > 1e-300)
    others = np.delete(np.arange(mesh.ncells), bad)
    assert np.all(np.abs(dc.cell_det(mesh, others)) > 0.0)
    healthy = dc.healthy(name)
    assert np.all(np.abs(dc.cell_det(healthy)) > 0.0)


def test_documented_geometry():
    mesh, bad = dc.case("collapsed")
    i, j = dc.SQUARE
    sq = (j * dc.N + i) * 4 + np.arange(4)
    assert sq[0] == bad
    assert np.array_equal(np.abs(dc.cell_det(mesh, sq)), [0.0, 2.0 ** -7, 2.0 ** -6, 2.0 ** -7])
    for off in dc.LIMIT_OFFSETS:
        m, b = dc.case("collapsed", off)
        assert dc.cell_det(m, b)[0] == off / dc.N ** 2 > 0.0
    # the sliver's long edge is a boundary facet / an interior facet
    for name, nb in (("sliver_boundary", 1), ("sliver", 0), ("sliver_hub", 0)):
        mesh, bad = dc.case(name)
        on_boundary = np.isin(mesh.cell_facets[bad], mesh.boundary_facets())
        assert on_boundary.sum() == nb


@pytest.mark.parametrize("name", NAMES)
def test_tile_classes_of_the_bad_patches(name):
    import tile_classes as tcl
    mesh, bad = dc.case(name)
    b, c = tcl.node_bins_classes(mesh)
    got = sorted((int(b[v]), int(c[v])) for v in mesh.cell_nodes[bad])
    expect = {"collapsed": [(0, 0), (1, 0), (1, 0)],        # full 4-cell patch, two full 8-cell patches
              "sliver": [(0, 1), (2, 4), (2, 4)],           # P - 1 class of bin 0, two interior patches of bin P = 16
              "sliver_boundary": [(0, 1), (1, 5), (1, 5)],  # ... two boundary patches of 6 facets
              "sliver_hub": [(0, 1), (1, 2), (5, 5)],       # the hub of 71 cells is beyond the bins
              "sliver_hub40": [(0, 1), (1, 2), (4, 4)]}[name]   # a 41-facet patch: bin P = 64
    if name == "sliver_hub":
        assert got[:2] == expect[:2] and got[2][0] == 5
    else:
        assert got == expect


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("name", NAMES)
def test_oracle_node_by_node_is_finite_and_unrestricted_refuses(oracle_mod, name, k):
    from synthetic import facet_types
    mesh, bad = dc.case(name)
    ft = facet_types(mesh)
    nd = k * (k + 1) // 2
    rng = np.random.default_rng(k)
    G, f = rng.standard_normal((1, mesh.ncells * nd * 2)), rng.standard_normal((1, mesh.ncells * nd))
    far = dc.far_cells(mesh, bad)
    if k == 1:
        # RT_1 has no patch matrix to factorise (one scalar, sum L / sum T): the reference does not notice the flat
        # cell, it divides and returns non-finite coefficients - on cells of the three bad patches only
        full = oracle_mod.se_reconstruct(mesh, k, ft, G, f).reshape(mesh.ncells, -1)
        assert not np.isfinite(full).all() and np.isfinite(full[far]).all()
    else:
        with pytest.raises(RuntimeError, match="status -2"):
            oracle_mod.se_reconstruct(mesh, k, ft, G, f)
    ref = np.zeros((1, mesh.ncells * k * (k + 2)))
    for node in np.nonzero(dc.good_mask(mesh, bad))[0]:
        oracle_mod.se_reconstruct(mesh, k, ft, G, f, flux_hdiv=ref, node_range=(int(node), int(node) + 1))
    assert np.isfinite(ref).all()
    ref = ref.reshape(mesh.ncells, -1)
    assert np.all(ref[bad] == 0.0)                       # no patch of the sum holds the bad cell
    assert np.abs(ref[far]).max() > 0.0
    if k == 1:
        assert np.array_equal(ref[far], full[far])       # the far cells hold the same sums either way
        return
    # a patch of the bad cell alone is what the oracle refuses
    for node in mesh.cell_nodes[bad]:
        with pytest.raises(RuntimeError, match="status -2"):
            oracle_mod.se_reconstruct(mesh, k, ft, G, f, node_range=(int(node), int(node) + 1))
