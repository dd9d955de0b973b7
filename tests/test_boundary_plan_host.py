"""The planner of eqlb_se_set_boundary on the host (no GPU): tools/boundary_plan_emul.cpp includes
dolfinx_eqlb_amd/csrc/eqlb_boundary_plan.h - the header the library plans its boundary tables with - and prints the
plan of a mesh and a facet-type table written to a text file here.  The plan is compared with a direct numpy statement:

  * bin = smallest of 4, 8, 16, 32, 64 >= facets at the node; more than 63 cells or 64 facets: a large patch;
  * inside a bin the patches in node order - the full ones (interior, as many cells as lanes) of the bins 0, 1 first
    where, and only where, the fused stress route applies (RT_2 stress, DG_1 data, no tractions, SE mode);
  * lane slots and patch indices as prefix sums over the bins;
  * large nodes ascending, CSR offsets = running cell counts, work-space offsets = running sums of the callback;
  * the cells of the compact reductions: those with a vertex in the node set;
  * groups of boundary patches and their levels: the discovery loop of se/reconstruction.hpp:170-234 written out.

Refusals come back with the code and the text of the C ABI.  The program is built as a plain executable with the
address and undefined-behaviour sanitizers where the compiler has them; it also checks that the planner wrote to
nothing but the plan."""

import os
import shutil
import subprocess

import numpy as np
import pytest

import cases
import topology_meshes as tm
from dolfinx_eqlb_amd.mesh import create_disk, create_unit_square
from synthetic import facet_types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = np.array([4, 8, 16, 32, 64])
INVALID, TOO_SMALL, UNSUPPORTED, TOO_LARGE = -1, -2, -3, -5      # include/eqlb.h


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("boundary_plan")
    exe = str(tmp / "boundary_plan_emul")
    base = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tools", "boundary_plan_emul.cpp"),
            "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True,
                         text=True)
    if san.returncode != 0:   # (a compiler without the sanitizer runtimes: the plans are still checked)
        subprocess.run(base, check=True)
    return exe, tmp


def plan(emul, mesh, ft, k=2, deg=None, stress=0, mode=0, large=0, large_stress=0, mask=None, bvalues=0, env=None):
    exe, tmp = emul
    ft = np.atleast_2d(ft)
    deg = k - 1 if deg is None else deg
    arrays = [[mesh.nnodes, mesh.ncells, mesh.nfacets, ft.shape[0]], [k, deg, stress, mode, large, large_stress],
              [int(mask is not None), bvalues], mesh.cell_nodes, mesh.facet_nodes, mesh.facet_cells_offsets,
              mesh.node_cells_offsets, mesh.node_cells, mesh.node_facets_offsets, mesh.node_facets, ft]
    if mask is not None:
        arrays.append(mask)
    path = str(tmp / "case.txt")
    with open(path, "w") as fh:
        for a in arrays:
            fh.write(" ".join(str(int(v)) for v in np.asarray(a).ravel()) + "\n")
    e = dict(os.environ)
    e.pop("EQLB_STRESS_MIXED_TILES", None)
    e.update(env or {})
    run = subprocess.run([exe, path], capture_output=True, text=True, env=e)
    assert run.returncode == 0, (run.returncode, run.stderr)
    out = {}
    for line in run.stdout.splitlines():
        key, _, rest = line.partition(" ")
        if key == "message":
            out[key] = rest
        elif key == "bin":
            out.setdefault("bins", []).append([int(v) for v in rest.split()])
        else:
            out[key] = np.array([int(v) for v in rest.split()], dtype=np.int64)
    return out


def counts(mesh):
    return np.diff(mesh.node_cells_offsets), np.diff(mesh.node_facets_offsets)


def touching(mesh, nodes):
    flag = np.zeros(mesh.nnodes, dtype=bool)
    flag[nodes] = True
    return np.nonzero(flag[mesh.cell_nodes].any(axis=1))[0]


def check_bins(mesh, got, mask=None, full_first=False):
    """The numpy statement of the bins; returns (node_bin, full)."""
    nc, nf = counts(mesh)
    on = np.ones(mesh.nnodes, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    b = np.searchsorted(P, nf, side="left")
    large = on & ((b == 5) | (nc > 63))
    node_bin = np.where(on & ~large, b, -1)
    full = (node_bin >= 0) & (nc == nf) & (nc == P[np.clip(node_bin, 0, 4)])
    first = full & (node_bin < 2) & full_first
    node_patch = -np.ones(mesh.nnodes, dtype=np.int64)
    node_slot = node_patch.copy()
    soff = poff = 0
    bins = []
    for bb in range(5):
        members = np.nonzero(node_bin == bb)[0]
        order = np.concatenate([members[first[members]], members[~first[members]]])
        node_patch[order] = poff + np.arange(order.size)
        node_slot[order] = soff + P[bb] * np.arange(order.size)
        bins.append([P[bb], order.size, soff, poff, int(first[members].sum())])
        soff += P[bb] * order.size
        poff += order.size
    assert np.array_equal(got["node_bin"], node_bin)
    assert np.array_equal(got["node_patch"], node_patch)
    assert np.array_equal(got["node_slot"], node_slot)
    assert got["bins"] == bins
    assert got["totals"][0] == soff and got["totals"][1] == poff
    ln = np.nonzero(large)[0]
    assert np.array_equal(got["large_nodes"], ln)
    if ln.size:
        assert np.array_equal(got["l_off"], np.concatenate([[0], np.cumsum(nc[ln])]))
        assert got["totals"][2] == nc[ln].max()
        assert np.array_equal(got["l_cells"], touching(mesh, ln))
    else:
        assert got["l_off"].size == 0 and got["l_cells"].size == 0 and got["totals"][2] == 0
    return node_bin, full


def flags(got):
    return dict(zip(("inhomogeneous", "stress_flux_bcs", "stress_fused_ok", "tiles", "t_stress", "t_mixed", "ws_levels",
                     "any"), (int(v) for v in got["flags"])))


# ------------------------------------------------------------------------------------------------ bins 0 and 1
@pytest.mark.parametrize("masked", [False, True])
def test_crossed_square(emul, masked):
    mesh = create_unit_square(2)
    nc, nf = counts(mesh)
    assert set(np.searchsorted(P, nf, side="left")) == {0, 1} and np.any(nc == nf) and np.any(nc != nf)
    ft = facet_types(mesh, None)
    mask = None
    if masked:      # a boundary node, an interior node of each bin
        mask = np.ones(mesh.nnodes, dtype=np.uint8)
        mask[[np.nonzero(nc != nf)[0][1], np.nonzero((nc == nf) & (nc == 4))[0][0], np.nonzero(nc == 8)[0][0]]] = 0
    for k in (2, 4):
        got = plan(emul, mesh, ft, k=k, mask=mask, bvalues=k // 2)
        assert got["code"][0] == 0
        node_bin, _ = check_bins(mesh, got, mask)
        fl = flags(got)
        # plain flux equilibration: tiles up to RT_3, and they list every patch of the bins (stress_fused_ok speaks of
        # degree and tractions only; t_stress is the route)
        assert fl == dict(inhomogeneous=int(k == 4), stress_flux_bcs=0, stress_fused_ok=int(k == 2), tiles=int(k <= 3),
                          t_stress=0, t_mixed=0, ws_levels=1, any=0)
        assert np.array_equal(got["tile_bin"], node_bin if k <= 3 else [])
        assert got["rest_cells"].size == 0 and got["l_rest_cells"].size == 0 and got["totals"][3] == 0
        assert got["ws"].size == 0 and got["group"].size == 0 and got["level"].size == 0


# ------------------------------------------------------------------------------------------------ full-first order
def test_hole_plain_and_stress(emul):
    mesh = tm.mesh_of("hole")
    ft = tm.facet_table(mesh, "dirichlet")
    check_bins(mesh, plan(emul, mesh, ft), full_first=False)
    ft2 = np.repeat(ft, 2, axis=0)
    for forced in (None, "0", "1"):
        env = {} if forced is None else {"EQLB_STRESS_MIXED_TILES": forced}
        got = plan(emul, mesh, ft2, stress=1, env=env)
        node_bin, full = check_bins(mesh, got, full_first=True)
        assert sum(b[4] for b in got["bins"]) > 0 and any(0 < b[4] < b[1] for b in got["bins"][:2])
        listed = (node_bin >= 0) & (node_bin < 2)
        nlisted = int(listed.sum())
        mixed = (20 * int((listed & ~full).sum()) > nlisted) if forced is None else forced == "1"
        fl = flags(got)
        assert (fl["stress_fused_ok"], fl["tiles"], fl["t_stress"], fl["t_mixed"]) == (1, 1, 1, int(mixed))
        rest = (node_bin >= 2) | ((node_bin >= 0) & ~full & (not mixed))
        assert np.array_equal(got["tile_bin"], np.where(rest, -1, node_bin))
        assert got["totals"][3] == rest.sum() and (rest.sum() > 0) == (not mixed)      # (no patch above 8 facets)
        assert np.array_equal(got["rest_cells"], touching(mesh, np.nonzero(rest)[0]))
        assert got["l_rest_cells"].size == 0
    # off the fused route - DG_0 data, tractions, EV mode - the bins are in plain node order and nothing is left out
    ftn = np.repeat(tm.facet_table(mesh, "flux_middle"), 2, axis=0)
    for kwargs in (dict(ft=ft2, stress=1, deg=0), dict(ft=ftn, stress=1), dict(ft=ft, mode=1)):
        got = plan(emul, mesh, **kwargs)
        node_bin, _ = check_bins(mesh, got, full_first=False)
        fl = flags(got)
        assert fl["t_stress"] == 0 and fl["tiles"] == int(not kwargs.get("stress", 0))
        assert fl["stress_flux_bcs"] == int(kwargs["ft"] is ftn) and fl["any"] == 0
        assert got["rest_cells"].size == 0


# ------------------------------------------------------------------------------------------------ large patches
def test_disk_hub(emul):
    mesh = create_disk(70, 1)
    nc, nf = counts(mesh)
    hub = int(np.argmax(nc))
    assert nc[hub] == 70 and np.count_nonzero(nc > 63) == 1
    ft = facet_types(mesh, None)
    ft2 = np.repeat(ft, 2, axis=0)
    refused = [
        (dict(ft=ft), TOO_LARGE, f"Patch around node {hub} has 70 cells (limit 63)"),
        (dict(ft=ft2, stress=1, large=1), TOO_LARGE,
         f"Patch around node {hub} has 70 cells: the stress equilibration (weak symmetry, Korn constants) is limited "
         "to 63 cells per patch, \"large_patches\" covers flux equilibration only"),
        (dict(ft=ft, k=4, mode=1, large=1), TOO_LARGE,
         f"Patch around node {hub} has 70 cells: the constrained minimisation at RT_4 is limited to 63 cells per "
         "patch, \"large_patches\" covers it for RT_1 ... RT_3"),
        (dict(ft=ft2, stress=1, large_stress=1), TOO_LARGE, f"Patch around node {hub} has 70 cells (limit 63)"),
    ]
    for kwargs, code, text in refused:
        got = plan(emul, mesh, **kwargs)
        assert got["code"][0] == code and got["message"] == text, got
    bad = ft.copy()
    bad[0, 3] = 3
    got = plan(emul, mesh, bad, large=1)
    assert got["code"][0] == INVALID and got["message"] == "eqlb_se_set_boundary: facet type 3 out of range"
    # accepted: masked out, or on a handle with "large_patches"
    mask = np.ones(mesh.nnodes, dtype=np.uint8)
    mask[hub] = 0
    got = plan(emul, mesh, ft, mask=mask)
    check_bins(mesh, got, mask)
    assert got["large_nodes"].size == 0
    got = plan(emul, mesh, ft, large=1)
    node_bin, _ = check_bins(mesh, got)
    assert np.array_equal(got["large_nodes"], [hub]) and np.array_equal(got["l_off"], [0, 70])
    assert got["l_wsym_off"].size == 0 and node_bin[hub] == -1 and got["tile_bin"][hub] == -1
    # stress: work-space offsets from the callback (2 n^2 + n doubles in the program); the fused route merges the cells
    # of the large patches into the list of the rest
    got = plan(emul, mesh, ft2, stress=1, large=1, large_stress=1)
    node_bin, full = check_bins(mesh, got, full_first=True)
    assert np.array_equal(got["l_wsym_off"], [0, 2 * 70 * 70 + 70])
    fl = flags(got)
    assert fl["t_stress"] == 1
    rest = (node_bin >= 2) | ((node_bin >= 0) & ~full & (not fl["t_mixed"]))
    assert np.array_equal(got["rest_cells"], touching(mesh, np.nonzero(rest)[0]))
    assert np.array_equal(got["l_rest_cells"], touching(mesh, np.nonzero(rest | (np.arange(mesh.nnodes) == hub))[0]))


# ------------------------------------------------------------------------------------------------ groups and levels
def groups_of(mesh, ft, mask=None):
    """ws, group, level, number of levels: the nodes in ascending order; a two-cell node with tractions on both of its
    boundary facets in both rows opens a group with the node across its interior facet and that node's other two-cell
    neighbours of the same kind; level of a group = 1 + the highest level among the earlier groups that own a vertex
    of a cell of its internal patch."""
    nn = mesh.nnodes
    nc, _ = counts(mesh)
    cnt = np.zeros(nn, dtype=int)
    for r in range(2):
        np.add.at(cnt, mesh.facet_nodes[ft[r] == 2].ravel(), 1)
    two = (cnt == 4) & (nc == 2)
    ws, group = np.zeros(nn, dtype=int), -np.ones(nn, dtype=int)
    inner_of = []
    cells_of = lambda n: mesh.node_cells[mesh.node_cells_offsets[n]:mesh.node_cells_offsets[n + 1]]  # noqa: E731
    for node in range(nn):
        if not two[node] or group[node] >= 0 or (mask is not None and not mask[node]):
            continue
        fcts = mesh.node_facets[mesh.node_facets_offsets[node]:mesh.node_facets_offsets[node + 1]]
        inner_f = fcts[ft[0][fcts] == 0]
        if inner_f.size == 0:
            continue
        a, b = mesh.facet_nodes[inner_f[0]]
        inner = int(b if a == node else a)
        members = {inner} | {int(n) for n in np.unique(mesh.cell_nodes[cells_of(inner)]) if two[n]}
        if len(members) < 2:
            continue
        assert all(group[n] < 0 for n in members)
        for n in members:
            group[n] = len(inner_of)
            ws[n] = 2 if n == inner else 1
        inner_of.append(inner)
    glevel = []
    for g, inner in enumerate(inner_of):
        earlier = [group[n] for n in np.unique(mesh.cell_nodes[cells_of(inner)]) if 0 <= group[n] < g]
        glevel.append(1 + max(glevel[e] for e in earlier) if earlier else 0)
    level = np.where(group >= 0, np.array(glevel + [0])[group], 0)
    return ws, group, level, max(glevel) + 1


@pytest.mark.parametrize("name", ["double_fan_0", "double_fan_1", "fan_chain"])
def test_groups_and_levels(emul, name):
    mesh = cases.fan_chain_mesh() if name == "fan_chain" else cases.double_fan_mesh(int(name[-1]))
    ft = np.repeat(facet_types(mesh, lambda p: np.ones(len(p), dtype=bool)), 2, axis=0)
    ws, group, level, nlevels = groups_of(mesh, ft)
    assert group.max() == 1 and np.count_nonzero(ws == 2) == 2 and np.count_nonzero(ws == 1) == 6
    assert nlevels == (1 if name == "fan_chain" else 2)      # overlapping internal patches: one after the other
    got = plan(emul, mesh, ft, stress=1)
    check_bins(mesh, got, full_first=False)
    fl = flags(got)
    assert (fl["stress_flux_bcs"], fl["t_stress"], fl["tiles"], fl["any"], fl["ws_levels"]) == (1, 0, 0, 1, nlevels)
    assert np.array_equal(got["ws"], ws) and np.array_equal(got["group"], group)
    assert np.array_equal(got["level"], level)
    # groups belong to RT_2: none are looked for at RT_3
    got = plan(emul, mesh, ft, k=3, stress=1)
    assert flags(got)["any"] == 0 and got["ws"].size == 0
    # a member that is masked out: the reference's refusal
    mask = np.ones(mesh.nnodes, dtype=np.uint8)
    mask[np.nonzero(ws == 1)[0][-1]] = 0
    got = plan(emul, mesh, ft, stress=1, mask=mask)
    assert got["code"][0] == UNSUPPORTED
    assert got["message"] == "Incompatible mesh! To many patches with 2 cells on neumann boundary."


@pytest.mark.parametrize("order", [0, 1])
def test_large_patch_in_a_group(emul, order):
    mesh = cases.big_double_fan_mesh(61, order)
    nc, _ = counts(mesh)
    hub = int(np.argmax(nc))
    assert nc[hub] == 64
    ft = np.repeat(facet_types(mesh, lambda p: np.ones(len(p), dtype=bool)), 2, axis=0)
    ws, group, _, _ = groups_of(mesh, ft)
    assert ws[hub] == 2
    got = plan(emul, mesh, ft, stress=1, large=1, large_stress=1)
    assert got["code"][0] == UNSUPPORTED
    assert got["message"] == (
        f"Patch around node {hub} has 64 cells and is the internal patch of group {group[hub]} of boundary patches "
        "with tractions on both stress rows: groups are limited to 63 cells per patch (\"large_patches_stress\")")
    # without tractions no groups: the same mesh is planned, the hub a large patch
    ftd = np.repeat(facet_types(mesh, None), 2, axis=0)
    got = plan(emul, mesh, ftd, stress=1, large=1, large_stress=1)
    check_bins(mesh, got, full_first=True)
    assert np.array_equal(got["large_nodes"], [hub])
