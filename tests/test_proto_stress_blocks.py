"""The banded weak-symmetry algorithm of eqlb_se_weaksym_banded.hip (numpy statement: proto_stress_blocks.py) against
the oracle's weak-symmetry corrections of single patches at RT_3 and RT_4 - large interior patches and boundary
patches with flux BCs on one and on both stress rows.  CPU only."""

import numpy as np
import pytest

import galerkin as gk
import proto_stress_blocks as pb
from test_gpu_stress_large_patches import flux_types, half_annulus


def patch_case(oracle_mod, mesh, k, ft, G, f, bv, node):
    """Oracle correction of the patch of `node` (stress minus row-wise result over that node alone), the numpy
    statement's correction from the row-wise result, and the flux-BC bits of the patch per row."""
    rows = oracle_mod.se_reconstruct(mesh, k, ft, G, f, boundary_values=bv, node_range=(node, node + 1))
    full = oracle_mod.se_reconstruct(mesh, k, ft, G, f, boundary_values=bv, node_range=(node, node + 1),
                                     stress=True)
    fan = oracle_mod.build_patches(mesh, ft)
    nrt = k * (k + 2)
    c0, c1 = rows[0].reshape(-1, nrt), rows[1].reshape(-1, nrt)
    n = int(fan["ncells"][node])
    fcts = fan["fcts"][node]
    interior = fan["cells"][node][0] >= 0
    bc0 = tuple(bool(not interior and ft[r, fcts[0]] == 2) for r in range(2))
    bcn = tuple(bool(not interior and ft[r, fcts[n]] == 2) for r in range(2))
    corr = pb.stress_correction(mesh, k, fan, node, c0, c1, bc0, bcn).reshape(2, -1)
    return full - rows, corr, n, interior, bc0, bcn


@pytest.mark.parametrize("k", [3, 4])
@pytest.mark.parametrize("ns", [12, 40])
def test_interior_patch(oracle_mod, k, ns):
    from dolfinx_eqlb_amd.mesh import create_disk
    from synthetic import facet_types, make_compatible_stress_data
    mesh = create_disk(ns, 2, shuffle_seed=3)
    node = int(np.argmax(np.diff(mesh.node_cells_offsets)))
    ft = np.repeat(facet_types(mesh, None), 2, axis=0)
    G, f = make_compatible_stress_data(mesh, k, ft)
    ref, corr, n, interior, _, _ = patch_case(oracle_mod, mesh, k, ft, G, f, None, node)
    assert interior and n == ns
    assert np.abs(ref).max() > 1e-6
    assert np.abs(corr - ref).max() <= 1e-10 * np.abs(ref).max()


@pytest.mark.parametrize("k,m", [(3, 12), (4, 12), (3, 40), (4, 40)])
@pytest.mark.parametrize("rows", ["one", "both"])
def test_boundary_patch_with_flux_bcs(oracle_mod, k, m, rows):
    mesh = half_annulus(m)
    straight = lambda p: np.abs(p[:, 1]) < 1e-12  # noqa: E731
    ft = flux_types(mesh, [straight, straight if rows == "both" else None])
    G, f, bv = gk.solve_elasticity(mesh, k, ft, seed=5 * m + k)
    ref, corr, n, interior, bc0, bcn = patch_case(oracle_mod, mesh, k, ft, G, f, bv, 0)
    assert not interior and n == m
    assert bc0[0] and bcn[0] and (bc0[1] and bcn[1]) == (rows == "both")
    assert np.abs(ref).max() > 1e-6
    assert np.abs(corr - ref).max() <= 1e-10 * np.abs(ref).max()
