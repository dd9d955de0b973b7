"""The oracle on vertex patches of more than 63 cells (the ground of the device's large-patch kernel, option
"large_patches"): divergence and jump predicates on polar disks with a hub of valence 64 ... 257 and on half annuli
whose hub lies on the boundary, and the hub patch against independent solutions of the same patch problem - what
test_oracle_high_valence_patch_is_the_minimiser does for valence 12.

HUB_DISCREPANCY records, per case and degree, by how much two double-precision solutions of the hub patch that
eliminate in different orders lie apart, relative to max |solution|:

* RT_1 ... RT_3: the oracle against the independent minimiser (tests/kkt_reference.py).  The numbers are those of
  the specification of these tests (its table of CPU measurements), not re-measured here; what this tree measures is
  printed by the tests and stays within the factor 10 (largest ratio: 7.2 on the half annulus 64 at RT_3).
* RT_4, which that table does not cover: the oracle against the numpy statement of the device formulation
  (tests/proto_gpu_math.py: the same reduced SPD system, solved densely by LAPACK) - two elimination orders on one
  problem, which is what the device adds a third to.  Measured on this tree when the tests were written, rounded up.
  The independent minimiser lies as far from either of them at RT_4 (1e-11 ... 2e-10, its KKT residual at 1e-14):
  on these fans fp64 does not pin the RT_4 patch solution below that level.

Every record is pinned by a test of this file: measured <= 10 x record.  tests/test_gpu_large_patches.py imports the
table for its device-vs-oracle bounds."""

import numpy as np
import pytest

import kkt_reference as kr
from dolfinx_eqlb_amd.eqlb import check_eqlb_conditions as chk
from dolfinx_eqlb_amd.mesh import create_disk, create_mesh
from synthetic import facet_types, make_compatible_data

# (mesh kind, hub valence, rings) -> {k: recorded discrepancy of the hub patch}; k <= 3: oracle vs minimiser, from the
# specification's table (row named per case); k = 4: oracle vs numpy statement, measured on this tree
HUB_DISCREPANCY = {
    ("disk", 70, 1): {1: 4.3e-15, 2: 4.8e-14, 3: 1.5e-12, 4: 1.9e-11},      # table row "disk 70, nr = 1"
    ("disk", 64, 2): {1: 6.3e-15, 2: 1.7e-13, 3: 7.4e-13, 4: 5.2e-12},      # table row "disk 64 ... 128, nr = 2"
    ("disk", 65, 2): {1: 6.3e-15, 2: 1.7e-13, 3: 7.4e-13, 4: 7.3e-12},      # table row "disk 64 ... 128, nr = 2"
    ("disk", 70, 2): {1: 6.3e-15, 2: 1.7e-13, 3: 7.4e-13, 4: 3.8e-12},      # table row "disk 64 ... 128, nr = 2"
    ("disk", 100, 2): {1: 6.3e-15, 2: 1.7e-13, 3: 7.4e-13, 4: 7.3e-11},     # table row "disk 64 ... 128, nr = 2"
    ("disk", 128, 2): {1: 6.3e-15, 2: 1.7e-13, 3: 7.4e-13, 4: 5.6e-11},     # table row "disk 64 ... 128, nr = 2"
    ("disk", 257, 2): {1: 1.5e-14, 2: 5.1e-13, 3: 3.0e-12, 4: 1.9e-10},     # table row "disk 257, nr = 2"
    ("annulus", 64, 2): {1: 1.4e-14, 2: 5.5e-14, 3: 3.8e-13, 4: 2.0e-12},   # table row "half annulus 64"
    ("annulus", 100, 2): {1: 1.4e-14, 2: 5.5e-14, 3: 2.7e-13, 4: 1.6e-11},  # table row "half annulus 100"
}


def hub_discrepancy(kind, n, nr, k):
    return HUB_DISCREPANCY[(kind, n, nr)][k]


def half_annulus(m):
    """Hub node 0 on the straight boundary with a fan of m cells, two rings of m + 1 nodes over the upper half
    plane (the mesh of tests/test_gpu_stress_large_patches.py)."""
    j = np.arange(m + 1)
    th = np.linspace(0.0, np.pi, m + 1) + 0.2 * np.pi / m * np.sin(2.3 * j) * (j % m > 0)
    a = 1 + np.arange(m + 1)
    b = 2 + m + np.arange(m + 1)
    x = np.concatenate([[[0.0, 0.0]], np.stack([np.cos(th), np.sin(th)], 1),
                        2.0 * np.stack([np.cos(th), np.sin(th)], 1)])
    cells = [[0, a[i], a[i + 1]] for i in range(m)]
    for i in range(m - 1):
        cells += [[a[i], b[i], a[i + 1]], [a[i + 1], b[i], b[i + 1]]]
    cells += [[a[m - 1], b[m - 1], b[m]], [a[m - 1], b[m], a[m]]]
    return create_mesh(x, np.array(cells, dtype=np.int32))


STRAIGHT_LAYOUTS = {
    "dirichlet": None,
    "flux_one_side": lambda p: (np.abs(p[:, 1]) < 1e-12) & (p[:, 0] > 0.0),
    "flux_both_sides": lambda p: np.abs(p[:, 1]) < 1e-12,
}


def disk_case(ns, nr, k, degree_dg=None, seed=7):
    """Polar disk, flux BC on the upper half of the rim; the hub has ns cells."""
    mesh = create_disk(ns, nr, shuffle_seed=seed)
    ft = facet_types(mesh, lambda x: x[:, 1] > 0.0)
    G, f = make_compatible_data(mesh, k, ft, degree_dg=degree_dg)
    return mesh, ft, G[None], f[None]


def annulus_case(m, k, layout="dirichlet", degree_dg=None):
    mesh = half_annulus(m)
    ft = facet_types(mesh, STRAIGHT_LAYOUTS[layout])
    G, f = make_compatible_data(mesh, k, ft, degree_dg=degree_dg)
    return mesh, ft, G[None], f[None]


def hub_node(mesh):
    return int(np.argmax(np.diff(mesh.node_cells_offsets)))


def check_predicates(mesh, k, x, G, f):
    res, nrm = chk.divergence_residual(mesh, k, x, G, f)
    assert res < 1e-10 * nrm
    assert chk.check_jump_condition(mesh, k, x, G, atol=1e-11)


def _check_case(oracle_mod, kind, n, nr, k, mesh, ft, G, f):
    assert np.diff(mesh.node_cells_offsets).max() == n
    x = oracle_mod.se_reconstruct(mesh, k, ft, G, f)[0]
    check_predicates(mesh, k, x, G[0], f[0])
    node = hub_node(mesh)
    cells, st, sol, u = oracle_mod.se_patch(mesh, k, ft, G, f, node)
    assert len(cells) == n
    if k <= 3:
        other = "minimiser"
        oc, ocoef, resid, _ = kr.solve_patch(mesh, k, node, ft, G[0], f[0])
        assert resid < 1e-11
    else:
        import proto_gpu_math as pg
        from gen_tables import tables_float
        other = "numpy statement"
        tab = tables_float(k, k - 1)
        nd = tab["nd"]
        oc, ocoef = pg.patch_solve(mesh, tab, oracle_mod.build_patches(mesh, ft), node, ft[0],
                                   G[0].reshape(mesh.ncells, nd, 2), f[0].reshape(mesh.ncells, nd))
    order = [list(oc).index(c) for c in cells]
    err = np.abs(sol[0] - ocoef[order]).max() / np.abs(sol[0]).max()
    print(f"{kind} {n} nr={nr} k={k}: oracle vs {other} {err:.2e} (record {hub_discrepancy(kind, n, nr, k):.1e})")
    assert err <= 10.0 * hub_discrepancy(kind, n, nr, k)


CASES = [("disk", 70, 1), ("disk", 64, 2), ("disk", 65, 2), ("disk", 70, 2), ("disk", 100, 2), ("disk", 128, 2),
         ("disk", 257, 2), ("annulus", 64, 2), ("annulus", 100, 2)]


@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("kind,n,nr", CASES, ids=[f"{c[0]}{c[1]}-nr{c[2]}" for c in CASES])
def test_oracle_large_patch(oracle_mod, kind, n, nr, k):
    mesh, ft, G, f = disk_case(n, nr, k) if kind == "disk" else annulus_case(n, k)
    _check_case(oracle_mod, kind, n, nr, k, mesh, ft, G, f)
