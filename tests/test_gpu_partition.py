"""The general node-ownership Partition (dolfinx_eqlb_amd/distributed.py) with the DEVICE as the per-rank solver.

tests/_dist_worker_general.py states "the union of the owned parts equals the single-domain result" on CPU ranks with
the oracle as the solver; every device test of the multi-GPU path uses StripPartition, whose rim is a straight column
of cells.  Here the ranks of a decomposition run one after the other in this process on one device (no
torch.distributed, no second process): each rank equilibrates the patches of the nodes it owns on its local mesh -
"every cell with a vertex I own" - and its rows are added to the global cells in numpy.  The sum over the ranks must
be the single-domain oracle result (1e-11 of the largest coefficient, tests/test_gpu_parity.py).

The rim of such a local mesh holds what no other device test has: non-owned vertices at which two separate fans of
local cells meet (the patch builder must not walk them) and non-owned vertices with one cell.  That they are present
is asserted: these asserts are conditions on the input.
"""

import numpy as np
import pytest

from topology_meshes import node_counts

pytestmark = pytest.mark.gpu
RTOL = 1e-11
WORLD = 3


@pytest.fixture(scope="module")
def cpp():
    from dolfinx_eqlb_amd import cpp as c
    assert c.device_count() >= 1, "GPU tests need a HIP device"
    return c


_DECOMP = {}


def decomposition(kind):
    """(global mesh, global facet types, [Partition of rank 0 ... WORLD - 1])"""
    if kind not in _DECOMP:
        from dolfinx_eqlb_amd import distributed as dd
        from dolfinx_eqlb_amd.mesh import create_unit_square
        from synthetic import facet_types
        if kind == "random":
            gmesh = create_unit_square(12, shuffle_seed=1, perturb=0.2)
            owner = np.random.default_rng(0).integers(0, WORLD, gmesh.nnodes)
        else:   # the angular sectors of tests/_dist_worker_general.py
            from _dist_worker_general import delaunay_mesh
            gmesh = delaunay_mesh(260, 3)
            ang = np.arctan2(gmesh.x[:, 1] - 0.5, gmesh.x[:, 0] - 0.5)
            owner = np.minimum(((ang + np.pi) / (2 * np.pi) * WORLD).astype(int), WORLD - 1)
        gft = facet_types(gmesh)
        parts = [dd.Partition(gmesh, owner, r, WORLD) for r in range(WORLD)]
        assert sum(int(p.node_mask.sum()) for p in parts) == gmesh.nnodes
        _DECOMP[kind] = (gmesh, gft, parts)
    return _DECOMP[kind]


def rim_nodes(part):
    """(pinched, one-cell) local nodes and whether each is owned."""
    n, nf, _ = node_counts(part.mesh)
    own = part.node_mask.astype(bool)
    return (nf - n >= 2), (n == 1), own


@pytest.mark.parametrize("kind", ["random", "sectors"])
def test_rim_of_the_local_meshes(kind):
    """Conditions on the input: the random owner puts pinched non-owned vertices on the rim of every rank, none of
    them owned; both owners leave non-owned vertices with one cell."""
    _, _, parts = decomposition(kind)
    one_total = 0
    for part in parts:
        assert part.mesh.ncells <= 450
        pinched, one, own = rim_nodes(part)
        print(f"  rank {part.rank}: {part.mesh.ncells} cells, {np.count_nonzero(pinched & ~own)} pinched non-owned "
              f"nodes, {np.count_nonzero(one & ~own)} one-cell non-owned nodes")
        assert not np.any(pinched & own) and not np.any(one & own)
        if kind == "random":
            assert np.count_nonzero(pinched & ~own) >= 1
        one_total += np.count_nonzero(one & ~own)
    assert one_total >= 1


def _rank_data(part, gG, gf, ncells):
    G = gG.reshape(ncells, -1)[part.cell_global].ravel()[None]
    f = gf.reshape(ncells, -1)[part.cell_global].ravel()[None]
    return G, f


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("kind", ["random", "sectors"])
def test_se_sum_over_ranks_equals_single_domain(cpp, oracle_mod, kind, k):
    from synthetic import make_compatible_data
    gmesh, gft, parts = decomposition(kind)
    nrt = k * (k + 2)
    gG, gf = make_compatible_data(gmesh, k, gft, seed=5)
    ref = oracle_mod.se_reconstruct(gmesh, k, gft, gG[None], gf[None])[0].reshape(gmesh.ncells, nrt)
    scale = np.abs(ref).max()
    for scatter in (0, 2):
        total = np.zeros((gmesh.ncells, nrt))
        for part in parts:
            G, f = _rank_data(part, gG, gf, gmesh.ncells)
            eq = cpp.SemiExplicitEquilibrator(cpp.DeviceMesh(part.mesh), k, 1)
            eq.set_option("scatter", scatter)
            eq.set_boundary(part.facet_types(gft), node_mask=part.node_mask)
            x = eq.equilibrate_host(G, f)
            assert np.array_equal(x, eq.equilibrate_host(G, f))
            total[part.cell_global] += x.reshape(part.mesh.ncells, nrt)
        print(f"  scatter {scatter}: sum over ranks - single domain {np.abs(total - ref).max() / scale:.3e}")
        assert np.abs(total - ref).max() <= RTOL * scale


@pytest.mark.parametrize("kind", ["random", "sectors"])
def test_ev_sum_over_ranks_equals_single_domain(cpp, oracle_mod, kind):
    from dolfinx_eqlb_amd.eqlb.conforming import conforming_dofmap, conforming_to_broken
    from synthetic import make_compatible_data
    k = 2
    nrt = k * (k + 2)
    gmesh, gft, parts = decomposition(kind)
    gG, gf = make_compatible_data(gmesh, k, gft, seed=5)
    gcd, gnd = conforming_dofmap(gmesh, k)
    ref = conforming_to_broken(gmesh, k, oracle_mod.ev_reconstruct(gmesh, k, gft, gG[None], gf[None], gcd, gnd)[0])
    ref = ref.reshape(gmesh.ncells, nrt)
    total = np.zeros((gmesh.ncells, nrt))
    for part in parts:
        G, f = _rank_data(part, gG, gf, gmesh.ncells)
        eq = cpp.ConstrainedMinEquilibrator(cpp.DeviceMesh(part.mesh), k, 1)
        eq.set_option("output", 1)
        eq.set_boundary(part.facet_types(gft), node_mask=part.node_mask)
        x = eq.equilibrate_host(G, f)
        assert np.array_equal(x, eq.equilibrate_host(G, f))
        total[part.cell_global] += x.reshape(part.mesh.ncells, nrt)
    print(f"  sum over ranks - single domain {np.abs(total - ref).max() / np.abs(ref).max():.3e}")
    assert np.abs(total - ref).max() <= RTOL * np.abs(ref).max()


@pytest.mark.parametrize("kind", ["random", "sectors"])
def test_export_on_a_rank(cpp, oracle_mod, kind):
    """The fans of the owned nodes are the oracle's; a pinched non-owned node is not walked: cell count, -1 fill.
    Only the random owner has pinched nodes (asserted below, and per rank in test_rim_of_the_local_meshes): the
    sectors, like every geometric owner, have none, and check the fans of the owned nodes alone."""
    _, gft, parts = decomposition(kind)
    for part in parts:
        mesh, ft = part.mesh, part.facet_types(gft)
        eq = cpp.SemiExplicitEquilibrator(cpp.DeviceMesh(mesh), 1, 1)
        eq.set_boundary(ft, node_mask=part.node_mask)
        dev = eq.export_patches()
        pinched, _, own = rim_nodes(part)
        for nd in np.nonzero(own)[0]:
            fan = oracle_mod.build_patches(mesh, ft, node_range=(int(nd), int(nd) + 1))
            assert dev["stride"] == fan["stride"]
            for key in ("ncells", "cells", "fcts", "fcts_local", "inodes_local"):
                assert np.array_equal(dev[key][nd], fan[key][0]), (part.rank, key, nd)
        n = np.diff(mesh.node_cells_offsets)
        assert np.any(pinched) == (kind == "random")
        for nd in np.nonzero(pinched)[0]:
            assert dev["ncells"][nd] == n[nd]
            for key in ("cells", "fcts", "fcts_local", "inodes_local", "reversed"):
                assert np.all(dev[key][nd] == -1), (part.rank, key, nd)
