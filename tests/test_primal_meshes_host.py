"""The numpy statements of the P_p solves (dolfinx_eqlb_amd/lsolver/primal.py, mesh/transfer.py: restrict_lagrange) against
an assembled matrix on the meshes of tests/primal_mesh_cases.py - a vertex of 100 cells, a pinched vertex, two
components, an unstructured mesh, tiny, huge, far-from-origin and stretched cells - and the restriction against the dense
P^T on the hierarchies disk70 and lshape_graded.  The checks and their bounds are those of tests/test_primal_host.py,
tests/test_primal_elasticity_host.py and tests/test_multilevel_host.py (primal_cases.check_statement,
elasticity_cases.check_statement, multilevel_cases.check_restriction): chain_terms with the mesh's own valence, no
tolerance chosen here.  This is the link below tests/test_gpu_primal_meshes.py, which holds the device to these
statements bit for bit on the same inputs.

Largest |diff| / bound seen: 0.71 (Poisson load, p = 4, delaunay); largest apply ratio 0.13 (Poisson, p = 4,
aspect1000)."""

import numpy as np
import pytest

import elasticity_cases as ec
import multilevel_cases as mc
import primal_cases as pc
import primal_mesh_cases as pm

MESHES = ["disk100", "bowtie", "two_parts", "delaunay", "tiny_far", "huge", "aspect1000"]
_WORST = {}
_P = {}


def _record(kind, name, p, ratios):
    for part, r in zip(("apply", "load", "diagonal"), ratios):
        if r > _WORST.get("ratio", -1.0):
            _WORST.update(ratio=r, where=f"{kind} {part}, p = {p}, {name}")
    print(f"largest |diff| / bound so far: {_WORST['ratio']:.3f} ({_WORST['where']})")


def test_the_mesh_table_has_its_counts():
    for name in pm.COUNTS:
        mesh = pm.mesh_of(name)
        assert (mesh.ncells, pm.valence(mesh)) == (pm.COUNTS[name][0], pm.COUNTS[name][2] or pm.valence(mesh))
    from dolfinx_eqlb_amd.lsolver.primal import lagrange_dofmap
    sq91 = pm.mesh_of("sq91")
    assert lagrange_dofmap(sq91, 3)[1] == 149605 > pm.ROWS_PER_PASS
    assert 2 * lagrange_dofmap(sq91, 2)[1] == 133226 > pm.ROWS_PER_PASS
    det = {n: np.abs(pc.cell_geometry(pm.mesh_of(n))[1]) for n in ("tiny_far", "huge", "aspect1000")}
    assert det["tiny_far"].max() < 1e-13 and det["huge"].min() > 1e6
    assert np.all(pm.mesh_of("tiny_far").x[:, :2] >= 250.0)
    # the shuffled local order leaves cells of either orientation on every mesh of the bit-for-bit table but the
    # Delaunay one, whose cells are all counter-clockwise
    for name in pm.SINGLE:
        d = pc.cell_geometry(pm.mesh_of(name))[1]
        assert (d.min() > 0.0) if name == "delaunay" else (d.min() < 0.0 < d.max()), name


@pytest.mark.parametrize("name", ["disk70", "hole", "lshape_graded", "sq6_two"])
def test_the_hierarchies_have_their_counts(name):
    meshes, links = pm.levels_host(name)       # (asserts LEVEL_COUNTS)
    assert [m.ncells for m in meshes] == pm.LEVEL_COUNTS[name][0]


@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_poisson_statement_equals_the_assembled_operator(name, p):
    _record("Poisson", name, p, pc.check_statement(pm.mesh_of(name), p, name))


@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("p", [2, 4])
def test_elasticity_statement_equals_the_assembled_operator(name, p):
    _record("elasticity", name, p, ec.check_statement(pm.mesh_of(name), p, True, name))


def _links():
    return [(name, l) for name in ("disk70", "lshape_graded") for l in range(len(pm.LEVEL_COUNTS[name][1]))]


@pytest.mark.parametrize("name,link", _links())
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_restriction_is_the_transpose(name, link, p):
    """every link of the two hierarchies, bs = 1 and 2 on one dense P"""
    meshes, links = pm.levels_host(name)
    mesh, mesh2 = meshes[link], meshes[link + 1]
    pcell, npf = links[link]
    P = mc.dense_prolongation(mesh, mesh2, pcell, npf, p)
    for bs in (1, 2):
        mc.check_restriction(mesh, mesh2, pcell, npf, p, bs, P=P, name=f"{name} link {link}")


@pytest.mark.parametrize("case", [c for c in pm.SINGLE_SOLVES if c[4] <= 200], ids=pm.case_id)
def test_single_level_counts_of_the_table_are_the_statements(case):
    """the cases of up to 200 iterations (about a second each); the longer ones by primal_mesh_cases.statement_counts"""
    problem, name, p, layout, count, _ = case
    op = pm.statement(problem, pm.mesh_of(name), p, layout)[0]
    b, _, start = pm.solve_data(op, problem, name, p, layout != "all")
    info = op.pcg(b, start, rtol=1e-10, maxit=2 * count)[1]
    assert info["converged"] == 1 and abs(info["iterations"] - count) <= pm.allowance(count)


@pytest.mark.parametrize("case", [c for c in pm.HIERARCHY_SOLVES if c[4] <= 200 and c[3] <= 3], ids=pm.case_id)
def test_hierarchy_counts_of_the_table_are_the_statements(case):
    problem, name, p, nlevels, count, _ = case
    H = pm.host_hierarchy(problem, name, p, nlevels)[0]
    b, _, start = pm.solve_data(H.ops[-1], problem, name, p)
    info = H.pcg(b, start, rtol=1e-10, maxit=2 * count)[1]
    assert info["converged"] == 1 and abs(info["iterations"] - count) <= pm.allowance(count)


def test_the_smallest_spaces_have_the_free_rows_of_the_table():
    """and the statement's PCG ends after as many steps as there are free rows (none: the start comes back)"""
    for name, p, free, iterations in pm.SMALLEST:
        op = pm.statement("poisson", pm.mesh_of(name), p)[0]
        assert int((~op.fixed).sum()) == free, (name, p)
        b, _, start = pm.solve_data(op, "poisson", name, p, True)
        u, info = op.pcg(b, start, rtol=1e-10, maxit=50)
        assert info["converged"] == 1 and info["breakdown"] == 0 and info["iterations"] == (iterations or 0), (name, p)
        if not free:
            assert np.array_equal(u, start)
