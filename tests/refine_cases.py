"""Inputs of the refinement tests (tests/test_refine_host.py, tests/test_gpu_refine.py): name -> (mesh, marked)."""

import numpy as np


def zigzag_strip(ncells, spacing):
    """Nodes j = 0 ... ncells + 1 at (s_j, j mod 2), s_{j+1} - s_j = spacing(j); cell j = (j, j+1, j+2), every second
    one reflected."""
    from dolfinx_eqlb_amd.mesh import create_mesh
    s = np.concatenate([[0.0], np.cumsum([spacing(j) for j in range(ncells + 1)])])
    x = np.stack([s, np.arange(ncells + 2) % 2], axis=1).astype(np.float64)
    j = np.arange(ncells)
    cells = np.stack([j, j + 1, j + 2], axis=1)
    cells[1::2] = cells[1::2, ::-1]
    return create_mesh(x, cells.astype(np.int32))


NAMES = ["triangle", "right1", "sq3_cell5", "sq3_all", "sq3_empty", "sq3_duplicates", "graded_first", "graded_last",
         "ties_last", "ties_first", "disk", "hole", "lshape", "two_parts"]
_CASES = {}


def case(name):
    if name in _CASES:
        return _CASES[name]
    from dolfinx_eqlb_amd.mesh import create_disk, create_mesh, create_unit_square
    if name == "triangle":
        mesh = create_mesh(np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]), np.array([[0, 1, 2]], dtype=np.int32))
        marked = [0]
    elif name == "right1":
        mesh, marked = create_unit_square(1, "right"), [0]
    elif name.startswith("sq3_"):
        mesh = create_unit_square(3, shuffle_seed=1)
        marked = {"cell5": [5], "all": list(range(mesh.ncells)), "empty": [], "duplicates": [30, 17, 17, 5, 5, 5, 2]}[name[4:]]
    elif name.startswith("graded_"):
        mesh = zigzag_strip(300, lambda j: 0.001 * (j + 1))
        marked = [0] if name == "graded_first" else [299]
    elif name.startswith("ties_"):
        mesh = zigzag_strip(70, lambda j: 0.1)
        marked = [69] if name == "ties_last" else [0]
    elif name == "disk":
        mesh, marked = create_disk(70, 2, shuffle_seed=3), [0, 100]
    else:
        from topology_meshes import mesh_of
        mesh = mesh_of(name)
        marked = list(range(0, mesh.ncells, 7))
    _CASES[name] = (mesh, np.array(marked, dtype=np.int32))
    return _CASES[name]


def sq40():
    from dolfinx_eqlb_amd.mesh import create_unit_square
    return create_unit_square(40, shuffle_seed=2, perturb=0.3)


def level_marks(ncells, level):
    """1/40 of the cells at random, fixed seed per level."""
    return np.random.default_rng(100 + level).choice(ncells, size=max(1, ncells // 40), replace=False).astype(np.int32)
