"""eqlb_se_estimate_stress_mu (cpp.estimate_stress with cell_pi1 / mu / cell_mu) on the device, bit for bit against
eqlb_se_estimate_stress: with no arrays and mu = 1 the new entry gives the bits of the old one; with a cell-wise pi_1 drawn
from three values and a random mu every cell's energy and wsym are the values of the old entry run with that cell's own
pi_1, divided by mu_T in numpy (one IEEE division), and node_asym is unchanged.  The data are those of
tests/estimator_cases.py on delaunay, disk100 and sq33 (4356 cells: 17 workgroups of 256 and 4 cells)."""

import numpy as np
import pytest

import estimator_cases as E
from test_gpu_primal_solve import bits

pytestmark = pytest.mark.gpu

MESHES = ("delaunay", "disk100", "sq33")
PI_VALUES = np.array([0.5, 1.0, 50.0])
_DM = {}


def device_mesh(name):
    from dolfinx_eqlb_amd import cpp
    if name not in _DM:
        _DM[name] = cpp.DeviceMesh(E.mesh_of(name))
    return _DM[name]


def mu_of(ncells, seed=41):
    """cell-wise mu: log-uniform in [1e-3, 1e3]"""
    return 10.0 ** (-3.0 + 6.0 * np.random.default_rng(seed).random(ncells))


@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_estimate_stress_mu_bit_for_bit(name, k):
    from dolfinx_eqlb_amd import cpp
    mesh, D, dm = E.mesh_of(name), E.data(name, k, k - 1), device_mesh(name)
    x2, korn = np.ascontiguousarray(D["x"][:2]), np.ascontiguousarray(D["korn"])
    nc = mesh.ncells
    # no arrays, mu = 1, through the new entry: the bits of estimate_stress
    for pi_1 in (1.0, 50.0):
        ref = cpp.estimate_stress(dm, k, x2, korn, pi_1)
        e, w, a = np.full(nc, np.nan), np.full(nc, np.nan), np.full(mesh.nnodes, np.nan)
        cpp.estimate_stress_mu_raw(dm, k, x2.ctypes.data, korn.ctypes.data, pi_1, None, 1.0, None, e.ctypes.data,
                                   w.ctypes.data, a.ctypes.data, cpp.MEM_HOST)
        for got, want in zip((e, w, a), ref):
            assert np.array_equal(bits(got), bits(want))
    # cell-wise pi_1 from three values, random mu
    pick = np.random.default_rng(E.seed_of("estimate-mu", name, k)).integers(0, 3, size=nc)
    pi1, mu = PI_VALUES[pick], mu_of(nc)
    assert np.unique(pick).size == 3
    runs = [cpp.estimate_stress(dm, k, x2, korn, float(v)) for v in PI_VALUES]
    energy = np.choose(pick, [r[0] for r in runs]) / mu
    wsym = np.choose(pick, [r[1] for r in runs]) / mu
    for call in range(2):                                     # two calls give the same bits
        e, w, a = cpp.estimate_stress(dm, k, x2, korn, cell_pi1=pi1, cell_mu=mu)
        assert np.array_equal(bits(e), bits(energy))
        assert np.array_equal(bits(w), bits(wsym))
        assert np.array_equal(bits(a), bits(runs[0][2]))      # node_asym does not know the coefficients
    # the scalars: mu = 4 divides exactly, cell_pi1 alone leaves mu = 1, mu alone keeps the scalar pi_1
    e4, w4, _ = cpp.estimate_stress(dm, k, x2, korn, 50.0, mu=4.0)
    assert np.array_equal(bits(e4), bits(runs[2][0] / 4.0)) and np.array_equal(bits(w4), bits(runs[2][1] / 4.0))
    ep, wp, _ = cpp.estimate_stress(dm, k, x2, korn, 7.0, cell_pi1=pi1)      # (the scalar is not read beside the array)
    assert np.array_equal(bits(ep), bits(np.choose(pick, [r[0] for r in runs])))
    assert np.array_equal(bits(wp), bits(np.choose(pick, [r[1] for r in runs])))
    em, wm, _ = cpp.estimate_stress(dm, k, x2, None, 1.0, cell_mu=mu)
    r1 = cpp.estimate_stress(dm, k, x2, None, 1.0)
    assert np.array_equal(bits(em), bits(r1[0] / mu)) and np.array_equal(bits(wm), bits(r1[1] / mu))


def test_estimate_stress_mu_in_device_memory_and_refusals():
    import torch
    from dolfinx_eqlb_amd import cpp
    name, k = "sq33", 3
    mesh, D, dm = E.mesh_of(name), E.data(name, k, k - 1), device_mesh(name)
    nc = mesh.ncells
    x2, korn = np.ascontiguousarray(D["x"][:2]), np.ascontiguousarray(D["korn"])
    pi1, mu = PI_VALUES[np.arange(nc) % 3], mu_of(nc, seed=5)
    ref = cpp.estimate_stress(dm, k, x2, korn, cell_pi1=pi1, cell_mu=mu)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    dx, dk, dp, dmu = t(x2), t(korn), t(pi1), t(mu)
    outs = [torch.full((n,), float("nan"), dtype=torch.float64, device=dev) for n in (nc, nc, mesh.nnodes)]
    torch.cuda.synchronize()
    cpp.estimate_stress_mu_raw(dm, k, dx.data_ptr(), dk.data_ptr(), 1.0, dp.data_ptr(), 1.0, dmu.data_ptr(),
                               *[o.data_ptr() for o in outs])
    torch.cuda.synchronize()
    for o, r in zip(outs, ref):
        assert np.array_equal(bits(o.cpu().numpy()), bits(r))
    # refusals name the cell or the argument; the next valid call works
    for value in (0.0, -1.0, float("nan"), float("inf")):
        bad = np.ones(nc)
        bad[11] = value
        with pytest.raises(RuntimeError, match=r"eqlb_se_estimate_stress_mu: cell_mu\[11\] = "):
            cpp.estimate_stress(dm, k, x2, korn, cell_mu=bad)
        with pytest.raises(RuntimeError, match="eqlb_se_estimate_stress_mu: mu = "):
            cpp.estimate_stress(dm, k, x2, korn, mu=value)
    bad = np.ones(nc)
    bad[2] = -1.0
    with pytest.raises(RuntimeError, match=r"eqlb_se_estimate_stress_mu: cell_pi1\[2\] = "):
        cpp.estimate_stress(dm, k, x2, korn, cell_pi1=bad)
    with pytest.raises(RuntimeError, match="Input sizes does not match"):
        cpp.estimate_stress(dm, k, x2, korn, cell_mu=np.ones(nc + 1))
    again = cpp.estimate_stress(dm, k, x2, korn, cell_pi1=pi1, cell_mu=mu)
    assert all(np.array_equal(bits(a), bits(r)) for a, r in zip(again, ref))
