"""eqlb_primal_value_dg (cpp.primal_value_dg, csrc/eqlb_primal_flux.hip) against its numpy statement
(lsolver.primal.value_dg): out[r][c][n] = coeff[c] sum_i PV<p,d>[n][i] u[r][cell_dofs[c][i]], ascending i, every product
rounded on its own - bit for bit for every (p, d), one and three right-hand sides, with and without the coefficient and
with a caller's table, on the launch shapes of tests/test_gpu_primal_flux.py (4, 64, 256 cells, an unstructured mesh that
is no multiple of 64, and 18 workgroups with a partial last one); an index out of range in both memory spaces; the raw
entry on a caller's non-blocking stream; the pybind module and local_projection."""

import numpy as np
import pytest

from dolfinx_eqlb_amd.lsolver import primal
from test_gpu_primal_flux import PAIRS, SHAPE_MESHES, device_mesh, dofs, named_mesh, nd_of, random_u

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cpp():
    from dolfinx_eqlb_amd import cpp as c
    assert c.device_count() >= 1, "GPU tests need a HIP device"
    return c


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def coeff_of(ncells, seed=1):
    k = np.random.default_rng(seed).uniform(0.0, 1000.0, ncells)
    k[::5] = 0.0
    return k


@pytest.mark.parametrize("nrhs", [1, 3])
@pytest.mark.parametrize("p,d", PAIRS)
def test_every_pair_on_every_launch_shape_bit_for_bit(cpp, p, d, nrhs):
    for name in SHAPE_MESHES:
        mesh = named_mesh(name)
        dm = device_mesh(cpp, name)
        cd, ndofs = dofs(name, p)
        u = random_u(name, p, nrhs, seed=7)
        kap = coeff_of(mesh.ncells)
        got = cpp.primal_value_dg(dm, p, d, cd, u)
        assert got.shape == (nrhs, mesh.ncells * nd_of(d))
        assert np.array_equal(bits(got), bits(primal.value_dg(p, d, cd, u))), name
        got = cpp.primal_value_dg(dm, p, d, cd, u, coeff=kap)
        assert np.array_equal(bits(got), bits(primal.value_dg(p, d, cd, u, kap))), name
        assert np.array_equal(bits(cpp.primal_value_dg(dm, p, d, cd, u, coeff=kap)), bits(got))   # two runs, the same bits
    # a single vector [ndofs] is one right-hand side
    if nrhs == 1:
        assert np.array_equal(bits(cpp.primal_value_dg(dm, p, d, cd, u[0], coeff=kap)), bits(got))


@pytest.mark.parametrize("p,d", [(1, 0), (2, 1), (3, 2), (4, 3), (4, 1), (2, 3)])
def test_op_hook(cpp, p, d):
    name = "unstructured"
    dm = device_mesh(cpp, name)
    mesh = named_mesh(name)
    cd, ndofs = dofs(name, p)
    u = random_u(name, p, 2, seed=3)
    kap = coeff_of(mesh.ncells, seed=2)
    ref = cpp.primal_value_dg(dm, p, d, cd, u, coeff=kap)
    builtin = cpp.get_value_table(p, d)
    assert np.array_equal(bits(cpp.primal_value_dg(dm, p, d, cd, u, coeff=kap, op=builtin)), bits(ref))
    # a caller's own table is used, in the caller's order of columns: the ascending sum over them
    own = np.random.default_rng(p + d).standard_normal((nd_of(d), nd_of(p)))
    got = cpp.primal_value_dg(dm, p, d, cd, u, coeff=kap, op=own)
    assert np.array_equal(bits(got), bits(primal.value_dg(p, d, cd, u, kap, op=own)))
    perm = np.roll(np.arange(nd_of(p))[::-1], 1)
    got = cpp.primal_value_dg(dm, p, d, cd[:, perm], u, op=builtin[:, perm])
    assert np.array_equal(bits(got), bits(primal.value_dg(p, d, cd[:, perm], u, op=builtin[:, perm])))
    with pytest.raises(RuntimeError, match="Input sizes does not match"):
        cpp.primal_value_dg(dm, p, d, cd, u, op=own.ravel()[:-1])


def test_refusals(cpp):
    name = "one_wave"
    dm = device_mesh(cpp, name)
    cd, ndofs = dofs(name, 2)
    u = random_u(name, 2, 1)
    for p, d in ((0, 1), (5, 1), (2, -1), (2, 4)):
        with pytest.raises(RuntimeError, match="degrees p = %d, degree_dg = %d" % (p, d)):
            cpp.primal_value_dg(dm, p, d, cd, u)
    with pytest.raises(RuntimeError, match="eqlb_primal_value_dg: nrhs = 0"):
        cpp.primal_value_dg_raw(dm, 2, 1, 0, cd.ctypes.data, ndofs, u.ctypes.data, None, u.ctypes.data,
                                memspace=cpp.MEM_HOST)
    with pytest.raises(RuntimeError, match="Input sizes does not match"):
        cpp.primal_value_dg(dm, 2, 1, cd[:-1], u)
    # host memory: an index out of range is refused by name before anything is launched
    bad = cd.copy()
    bad[17, 4] = ndofs
    with pytest.raises(RuntimeError, match=r"eqlb_primal_value_dg: cell_dofs\[17\]\[4\] = %d outside \[0, %d\)"
                                           % (ndofs, ndofs)):
        cpp.primal_value_dg(dm, 2, 1, bad, u)
    bad = cd.copy()
    bad[3, 0] = -1
    with pytest.raises(RuntimeError, match=r"cell_dofs\[3\]\[0\] = -1"):
        cpp.primal_value_dg(dm, 2, 1, bad, u)


def test_bad_index_in_device_memory_gives_nan_for_that_cell(cpp):
    import torch
    p, d, name = 2, 1, "one_block"
    mesh = named_mesh(name)
    dm = device_mesh(cpp, name)
    cd, ndofs = dofs(name, p)
    u = random_u(name, p, 2, seed=6)
    kap = coeff_of(mesh.ncells)
    ref = primal.value_dg(p, d, cd, u, kap).reshape(2, mesh.ncells, -1)
    bad = cd.copy()
    bad[17, 4] = ndofs
    bad[200, 0] = -1
    bad[255, 5] = 2 ** 31 - 1
    dev = "cuda:0"
    cd_d, u_d, k_d = [torch.from_numpy(np.array(a)).to(dev) for a in (bad, u, kap)]
    out = torch.zeros((2, mesh.ncells, nd_of(d)), dtype=torch.float64, device=dev)
    cpp.primal_value_dg_raw(dm, p, d, 2, cd_d.data_ptr(), ndofs, u_d.data_ptr(), k_d.data_ptr(), out.data_ptr(),
                            stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    good = np.ones(mesh.ncells, dtype=bool)
    good[[17, 200, 255]] = False
    assert np.isnan(got[:, ~good]).all() and np.array_equal(bits(got[:, good]), bits(ref[:, good]))


@pytest.mark.parametrize("p,d,nrhs", [(2, 1, 1), (3, 2, 3), (1, 1, 2), (4, 0, 2)])
def test_raw_entry_on_a_stream_equals_the_statement(cpp, p, d, nrhs):
    """the inputs exist only late on the caller's non-blocking stream (behind a spin kernel; before that the buffers hold
    NaN): what the call enqueues is ordered on THAT stream"""
    import torch
    name = "many_blocks"
    mesh = named_mesh(name)
    dm = device_mesh(cpp, name)
    cd, ndofs = dofs(name, p)
    u = random_u(name, p, nrhs, seed=4)
    kap = coeff_of(mesh.ncells, seed=3)
    ref = primal.value_dg(p, d, cd, u, kap)
    dev = "cuda:0"
    cd_d, u_src, k_d = [torch.from_numpy(np.array(a)).to(dev) for a in (cd, u, kap)]
    u_d = torch.full_like(u_src, float("nan"))
    stream = torch.cuda.Stream()  # non-blocking: not ordered against the default stream
    torch.cuda.synchronize()
    runs = []
    with torch.cuda.stream(stream):
        torch.cuda._sleep(20_000_000)
        u_d.copy_(u_src)
        for _ in range(2):
            out = torch.full((nrhs, mesh.ncells * nd_of(d)), float("nan"), dtype=torch.float64, device=dev)
            cpp.primal_value_dg_raw(dm, p, d, nrhs, cd_d.data_ptr(), ndofs, u_d.data_ptr(), k_d.data_ptr(),
                                    out.data_ptr(), stream=stream.cuda_stream)
            runs.append(out)
        u_d.fill_(float("nan"))
    stream.synchronize()
    a, b = [o.cpu().numpy() for o in runs]
    assert np.array_equal(bits(a), bits(ref)) and np.array_equal(bits(b), bits(ref))


def test_pybind_module_and_local_projection(cpp):
    from dolfinx_eqlb_amd.eqlb import _adapter
    from dolfinx_eqlb_amd.lsolver import PrimalFlux, PrimalValue, local_projection
    name, p, d = "unstructured", 3, 2
    mesh = named_mesh(name)
    cd, ndofs = dofs(name, p)
    u = random_u(name, p, 3, seed=9)
    kap = coeff_of(mesh.ncells)
    ref = primal.value_dg(p, d, cd, u, kap)
    cm = _adapter.module()
    assert np.array_equal(bits(cm.primal_value_dg(_adapter.cpp_mesh(mesh), p, d, cd, u, kap)), bits(ref))
    assert np.array_equal(bits(cm.primal_value_dg(_adapter.cpp_mesh(mesh), p, d, cd, u[0])),
                          bits(primal.value_dg(p, d, cd, u[0])))
    # a third data kind of local_projection, bs = 1, beside the others
    f = lambda x, y: np.sin(x) * y   # noqa: E731
    out = local_projection(mesh, d, [PrimalValue(p, cd, u[1], kap), f, PrimalValue(p, cd, u[2])], bs=1)
    assert len(out) == 3 and np.array_equal(bits(out[0]), bits(ref[1]))
    assert np.array_equal(bits(out[2]), bits(primal.value_dg(p, d, cd, u[2])[0]))
    assert np.array_equal(bits(out[1]), bits(local_projection(mesh, d, [f], bs=1)[0]))
    with pytest.raises(RuntimeError, match="Input sizes does not match"):
        local_projection(mesh, d, [PrimalValue(p, cd, u[1])], bs=2)
    with pytest.raises(RuntimeError, match="Input sizes does not match"):
        local_projection(mesh, d, [PrimalFlux(u[1], cd, p)], bs=1)
