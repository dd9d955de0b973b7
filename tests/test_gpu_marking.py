"""Marking on the device (eqlb_indicator_total, eqlb_mark_doerfler) against the numpy statement of
dolfinx_eqlb_amd/eqlb/marking.py: set for set on tie-free indicators at every size where a kernel changes its
shape (below a wave, a block, the block limit of the streaming kernels, not a multiple of either), the tie rule,
the np.isclose branch and the argument errors, bitwise reproducibility on a caller's stream, the combination
rule of the indicator, and the chain equilibrate -> estimate -> indicator -> marking in device memory.

The device sums in a fixed tree order, the host model sequentially.  Either order is off by at most
n 2^-53 = 1.1e-10 (n = 10^6) relative to the total, so the two can disagree where the running sum comes closer
than that to the cut-off.  Every case therefore asserts its own margin first - the distance of the running sum at
the break point, and one cell before it, from the cut-off, relative to the total - to be >= 1e-9 (9 x that
rounding); the worst margin of the 216 cases below is 3.1e-9."""

import functools

import numpy as np
import pytest

from dolfinx_eqlb_amd.eqlb import doerfler_marking
from dolfinx_eqlb_amd.eqlb.marking import indicator_total as indicator_total_model

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 4095, 4097, 100003, 1000000]
THETAS = [0.01, 0.3, 0.5, 0.6, 0.9, 0.999]
SENTINEL = -7
MARGIN = 1e-9


@pytest.fixture(scope="module")
def cpp():
    from dolfinx_eqlb_amd import cpp as c
    assert c.device_count() >= 1, "GPU tests need a HIP device"
    return c


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


@functools.lru_cache(maxsize=4)
def lognormal_case(ncells, s):
    """Indicators, their descending order (equal values in ascending id) and the sequential running sum."""
    eta = np.random.default_rng(20241003 + s).lognormal(0, 2, ncells)
    assert np.unique(eta).size == ncells  # tie-free
    order = np.argsort(-eta, kind="stable")
    running = np.cumsum(eta[order])
    for a in (eta, order, running):
        a.setflags(write=False)
    return eta, order, running


def model_with_margin(eta, order, running, theta):
    """(sorted marked ids, margin): the rule of doerfler_marking on the shared running sum, and the smaller distance
    of the running sum at the break point and one cell before it from the cut-off, relative to the total."""
    total = np.sum(eta)
    cutoff = theta * total
    over = np.flatnonzero(running > cutoff)
    assert over.size, "the cut-off is exceeded by some prefix"
    bp = int(over[0])
    before = running[bp - 1] if bp > 0 else 0.0
    margin = min(abs(running[bp] - cutoff), abs(before - cutoff)) / total
    return np.sort(order[:bp + 1]).astype(np.int32), margin


@functools.lru_cache(maxsize=4)
def _device_copy(ncells, s):
    import torch as t
    return t.from_numpy(np.array(lognormal_case(ncells, s)[0])).to("cuda:0")


def device_mark(cpp, torch, eta_d, theta, stream=None):
    """eqlb_mark_doerfler on device memory: (marked [ncells] with the sentinel behind the list, nmarked, total)."""
    n = eta_d.numel()
    dev = eta_d.device
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream())
    with ctx:
        marked = torch.full((n,), SENTINEL, dtype=torch.int32, device=dev)
        nm = torch.full((1,), -99, dtype=torch.int64, device=dev)
        tot = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
        cpp.mark_doerfler_raw(n, eta_d.data_ptr(), theta, marked.data_ptr(), nm.data_ptr(), tot.data_ptr(),
                              stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return marked.cpu().numpy(), int(nm.item()), float(tot.item())


# ------------------------------------------------------------------------------------- 1. against the host model
@pytest.mark.parametrize("theta", THETAS)
@pytest.mark.parametrize("s", [0, 1, 2])
@pytest.mark.parametrize("ncells", SIZES)
def test_marked_set_equals_host_model(cpp, torch, ncells, s, theta):
    eta, order, running = lognormal_case(ncells, s)
    ref, margin = model_with_margin(eta, order, running, theta)
    print(f"  n = {ncells}, seed {s}, theta = {theta}: {ref.size} marked, margin {margin:.3e}")
    assert margin >= MARGIN, "the inputs of this case were changed"
    if ncells <= 4097:
        assert np.array_equal(ref, doerfler_marking(eta, theta))
    marked, nm, total = device_mark(cpp, torch, _device_copy(ncells, s), theta)
    assert nm == ref.size
    assert np.array_equal(marked[:nm], ref)
    assert np.all(marked[nm:] == SENTINEL)
    assert abs(total - np.sum(eta)) <= 1e-13 * np.sum(eta)


# ------------------------------------------------------------------------------------------------------- 2. ties
def test_all_cells_equal_marks_the_lowest_ids(cpp, torch):
    eta = np.ones(257)
    ref = doerfler_marking(eta, 0.5)
    assert np.array_equal(ref, np.arange(129))
    marked, nm, total = device_mark(cpp, torch, torch.from_numpy(eta).to("cuda:0"), 0.5)
    assert nm == 129 and np.array_equal(marked[:nm], ref) and np.all(marked[nm:] == SENTINEL)
    assert total == 257.0
    got, tot = cpp.mark_doerfler(eta, 0.5)
    assert np.array_equal(got, ref) and tot == 257.0


@pytest.mark.parametrize("ncells", [65, 4097])
def test_value_repeated_across_the_threshold(cpp, torch, ncells):
    """8 > 2 = ... = 2 > 0.25 in shuffled positions (all sums are exact): the cut-off falls inside the twos."""
    rng = np.random.default_rng(ncells)
    na, nb = ncells // 8, ncells // 2
    eta = np.concatenate([np.full(na, 8.0), np.full(nb, 2.0), np.full(ncells - na - nb, 0.25)])
    eta = eta[rng.permutation(ncells)]
    take = nb // 2 + 1  # twos in the list
    theta = (8.0 * na + 2.0 * (take - 1) + 1.0) / eta.sum()
    big, tied = np.flatnonzero(eta == 8.0), np.flatnonzero(eta == 2.0)
    ref = doerfler_marking(eta, theta)
    assert np.array_equal(ref, np.sort(np.concatenate([big, tied[:take]])))
    marked, nm, _ = device_mark(cpp, torch, torch.from_numpy(eta).to("cuda:0"), theta)
    assert nm == na + take
    assert np.isin(big, marked[:nm]).all()                      # every value above t
    assert np.array_equal(np.setdiff1d(marked[:nm], big), tied[:take])  # the tied picks are the lowest ids
    assert np.array_equal(marked[:nm], ref) and np.all(marked[nm:] == SENTINEL)
    assert np.array_equal(cpp.mark_doerfler(eta, theta)[0], ref)


def test_all_zero_and_one_dominant_cell(cpp, torch):
    for eta in (np.zeros(300), np.array([0.0, -0.0, 0.0])):
        marked, nm, total = device_mark(cpp, torch, torch.from_numpy(eta).to("cuda:0"), 0.5)
        assert nm == eta.size and np.array_equal(marked, np.arange(eta.size)) and total == 0.0
    eta = np.full(1000, 1e-3)
    eta[617] = 10.0
    marked, nm, _ = device_mark(cpp, torch, torch.from_numpy(eta).to("cuda:0"), 0.5)
    assert nm == 1 and marked[0] == 617 and np.all(marked[1:] == SENTINEL)
    assert np.array_equal(cpp.mark_doerfler(eta, 0.5)[0], [617])


# ----------------------------------------------------------------------- 3. the isclose branch and argument errors
@pytest.mark.parametrize("theta", [1.0, 1.0 - 1e-9])
def test_theta_close_to_one_marks_every_cell(cpp, torch, theta):
    for ncells in (1, 65, 100003):
        eta = lognormal_case(ncells, 0)[0]
        marked, nm, total = device_mark(cpp, torch, _device_copy(ncells, 0), theta)
        assert nm == ncells and np.array_equal(marked, np.arange(ncells, dtype=np.int32))
        assert abs(total - np.sum(eta)) <= 1e-13 * np.sum(eta)
        got, _ = cpp.mark_doerfler(eta, theta)
        assert np.array_equal(got, np.arange(ncells))


def test_invalid_arguments_touch_nothing(cpp, torch):
    eta = np.array(lognormal_case(65, 0)[0])
    eta_d = _device_copy(65, 0)
    cases = [(65, 0.0), (65, -0.25), (65, 1.1), (65, float("nan")), (0, 0.5)]
    for ncells, theta in cases:
        marked, nm, tot = np.full(65, SENTINEL, dtype=np.int32), np.full(1, -99, dtype=np.int64), np.full(1, -3.0)
        with pytest.raises(RuntimeError, match="eqlb_mark_doerfler"):
            cpp.mark_doerfler_raw(ncells, eta.ctypes.data, theta, marked.ctypes.data, nm.ctypes.data, tot.ctypes.data,
                                  cpp.MEM_HOST)
        assert np.all(marked == SENTINEL) and nm[0] == -99 and tot[0] == -3.0
        marked_d = torch.full((65,), SENTINEL, dtype=torch.int32, device="cuda:0")
        nm_d = torch.full((1,), -99, dtype=torch.int64, device="cuda:0")
        tot_d = torch.full((1,), -3.0, dtype=torch.float64, device="cuda:0")
        with pytest.raises(RuntimeError, match="eqlb_mark_doerfler"):
            cpp.mark_doerfler_raw(ncells, eta_d.data_ptr(), theta, marked_d.data_ptr(), nm_d.data_ptr(),
                                  tot_d.data_ptr())
        torch.cuda.synchronize()
        assert bool((marked_d == SENTINEL).all()) and int(nm_d.item()) == -99 and float(tot_d.item()) == -3.0
    with pytest.raises(RuntimeError):
        cpp.mark_doerfler(np.zeros(0), 0.5)
    with pytest.raises(RuntimeError, match="eqlb_mark_doerfler"):
        cpp.mark_doerfler_raw(65, eta.ctypes.data, 0.5, None, None, None, cpp.MEM_HOST)


@pytest.mark.parametrize("bad", [float("nan"), -1.0, -1e-300])
def test_negative_or_nan_indicator(cpp, torch, bad):
    for ncells, where in ((65, 17), (4097, 4096)):
        eta = np.array(lognormal_case(ncells, 1)[0])
        eta[where] = bad
        if where > 30:
            eta[where - 30] = bad  # the message names the first one
        first = where - 30 if where > 30 else where
        marked, nm = np.full(ncells, SENTINEL, dtype=np.int32), np.full(1, -99, dtype=np.int64)
        with pytest.raises(RuntimeError, match=f"cell {first}$"):
            cpp.mark_doerfler_raw(ncells, eta.ctypes.data, 0.5, marked.ctypes.data, nm.ctypes.data, None,
                                  cpp.MEM_HOST)
        assert np.all(marked == SENTINEL) and nm[0] == -99
        marked_d, nm_d, _ = device_mark(cpp, torch, torch.from_numpy(eta).to("cuda:0"), 0.5)
        assert nm_d == -1 and np.all(marked_d == SENTINEL)


# ------------------------------------------------------------------------------- 4. reproducibility and streams
@pytest.mark.parametrize("ncells", [100003, 1000000])
def test_bitwise_reproducible_on_a_user_stream(cpp, torch, ncells):
    eta = lognormal_case(ncells, 2)[0]
    eta_d = _device_copy(ncells, 2)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=eta_d.device)
    runs = [device_mark(cpp, torch, eta_d, 0.6, stream=s) for _ in range(3)]
    for marked, nm, total in runs[1:]:
        assert nm == runs[0][1] and np.array_equal(marked, runs[0][0])
        assert np.float64(total).tobytes() == np.float64(runs[0][2]).tobytes()
    marked, nm, total = runs[0]
    assert 0 < nm < ncells and np.all(marked[nm:] == SENTINEL)
    got, tot = cpp.mark_doerfler(eta, 0.6)  # host memory space
    assert np.array_equal(got, marked[:nm]) and np.float64(tot).tobytes() == np.float64(total).tobytes()


# -------------------------------------------------------------------------------------------- 5. indicator_total
def device_indicator(cpp, torch, terms_d, pair, want_cell=True, want_totals=True):
    n, nt = terms_d[0].numel(), len(terms_d)
    cell = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")
    tot = torch.full((nt + 2,), float("nan"), dtype=torch.float64, device="cuda:0")
    cpp.indicator_total_raw(n, [t.data_ptr() for t in terms_d], pair, cell.data_ptr() if want_cell else None,
                            tot.data_ptr() if want_totals else None,
                            stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return cell.cpu().numpy(), tot.cpu().numpy()


@pytest.mark.parametrize("pair", [False, True], ids=["plain", "pair"])
@pytest.mark.parametrize("nterms", [1, 2, 3, 4])
@pytest.mark.parametrize("ncells", [1, 65, 4097, 100003])
def test_indicator_total(cpp, torch, ncells, nterms, pair):
    terms = np.random.default_rng(77 + nterms).lognormal(0, 2, (nterms, ncells))
    terms_d = [torch.from_numpy(t).to("cuda:0") for t in terms]
    if pair and nterms < 2:
        with pytest.raises(RuntimeError, match="eqlb_indicator_total"):
            cpp.indicator_total_raw(ncells, [t.data_ptr() for t in terms_d], True, None, None)
        with pytest.raises(RuntimeError, match="eqlb_indicator_total"):
            cpp.indicator_total(terms, True)
        return
    ref_cell, ref_tot = indicator_total_model(terms, pair)
    if pair and nterms == 2:  # demo/poisson/demo_error_estimation.py:117-119 as it stands
        assert np.array_equal(ref_cell, terms[0] + terms[1] + 2 * np.multiply(np.sqrt(terms[0]), np.sqrt(terms[1])))
    cell, tot = device_indicator(cpp, torch, terms_d, pair)
    assert np.all(np.abs(cell - ref_cell) <= 4 * np.spacing(ref_cell))
    assert np.all(np.abs(tot[:nterms + 1] - ref_tot) <= 1e-13 * ref_tot) and np.isnan(tot[nterms + 1])
    # bitwise repeatable, and each output on its own
    cell2, tot2 = device_indicator(cpp, torch, terms_d, pair)
    assert cell.tobytes() == cell2.tobytes() and tot.tobytes() == tot2.tobytes()
    cell3, tot3 = device_indicator(cpp, torch, terms_d, pair, want_totals=False)
    assert cell3.tobytes() == cell.tobytes() and np.isnan(tot3).all()
    cell4, tot4 = device_indicator(cpp, torch, terms_d, pair, want_cell=False)
    assert np.isnan(cell4).all() and tot4.tobytes() == tot.tobytes()
    # host memory space: the same bits
    hcell, htot = cpp.indicator_total(terms, pair)
    assert hcell.tobytes() == cell.tobytes() and htot.tobytes() == tot[:nterms + 1].tobytes()
    only_tot = np.full(nterms + 1, np.nan)
    cpp.indicator_total_raw(ncells, [t.ctypes.data for t in terms], pair, None, only_tot.ctypes.data, cpp.MEM_HOST)
    assert only_tot.tobytes() == htot.tobytes()
    only_cell = np.full(ncells, np.nan)
    cpp.indicator_total_raw(ncells, [t.ctypes.data for t in terms], pair, only_cell.ctypes.data, None, cpp.MEM_HOST)
    assert only_cell.tobytes() == hcell.tobytes()


def test_indicator_total_argument_errors(cpp, torch):
    t = torch.ones(8, dtype=torch.float64, device="cuda:0")
    for ncells, nterms in ((0, 1), (8, 0), (8, 9)):
        with pytest.raises(RuntimeError, match="eqlb_indicator_total"):
            cpp.indicator_total_raw(ncells, [t.data_ptr()] * nterms, False, None, None)
    cell, tot = device_indicator(cpp, torch, [t] * 8, True)  # the limit of 8 terms
    assert np.array_equal(cell, np.full(8, 10.0)) and np.array_equal(tot[:9], [8.0] * 8 + [80.0])


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_equilibrate_estimate_mark_in_device_memory(cpp, torch):
    """8 x 8 crossed square, P_2 Galerkin solution: equilibrate (SE, RT_2) -> eqlb_se_estimate + eqlb_oscillation ->
    eqlb_indicator_total(pair_last_two) -> eqlb_mark_doerfler(0.5); nothing leaves the device in between."""
    import galerkin as gk
    from dolfinx_eqlb_amd.elmtlib.quadrature import make_quadrature_triangle
    from dolfinx_eqlb_amd.eqlb import check_eqlb_conditions as chk
    from dolfinx_eqlb_amd.mesh import create_unit_square
    from synthetic import facet_types
    from test_estimator_bound import f_ex
    k, theta = 2, 0.5
    mesh = create_unit_square(8, shuffle_seed=3)
    nc = mesh.ncells
    fh = gk.project_rhs(mesh, k, f_ex)[0]
    u, cd = gk.solve_poisson(mesh, k, f_ex)
    G = gk.discrete_flux(mesh, k, u, cd)
    qp, qw = make_quadrature_triangle(8)
    J = chk.cell_geometry(mesh)[0]
    xq = mesh.x[mesh.cell_nodes[:, 0], :2][:, None, :] + np.einsum("cij,qj->cqi", J, qp)
    fv = f_ex(xq[..., 0], xq[..., 1])
    dm = cpp.DeviceMesh(mesh)
    se = cpp.SemiExplicitEquilibrator(dm, k, 1)
    se.set_boundary(facet_types(mesh, None))
    dev = "cuda:0"
    G_d, f_d, fv_d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (G, fh, fv)]
    x_d = torch.zeros(nc * k * (k + 2), dtype=torch.float64, device=dev)
    sig_d, osc_d, eta_d = [torch.full((nc,), float("nan"), dtype=torch.float64, device=dev) for _ in range(3)]
    tot_d = torch.full((3,), float("nan"), dtype=torch.float64, device=dev)
    marked_d = torch.full((nc,), SENTINEL, dtype=torch.int32, device=dev)
    nm_d = torch.full((1,), -99, dtype=torch.int64, device=dev)
    sum_d = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    se.equilibrate_device(G_d.data_ptr(), f_d.data_ptr(), x_d.data_ptr(), st)
    cpp.estimate_raw(dm, k, 1, x_d.data_ptr(), G_d.data_ptr(), f_d.data_ptr(), None, sig_d.data_ptr(), None, stream=st)
    cpp.oscillation_raw(dm, k, 1, x_d.data_ptr(), G_d.data_ptr(), qp, qw, fv_d.data_ptr(), None, osc_d.data_ptr(),
                        stream=st)
    cpp.indicator_total_raw(nc, [sig_d.data_ptr(), osc_d.data_ptr()], True, eta_d.data_ptr(), tot_d.data_ptr(),
                            stream=st)
    cpp.mark_doerfler_raw(nc, eta_d.data_ptr(), theta, marked_d.data_ptr(), nm_d.data_ptr(), sum_d.data_ptr(),
                          stream=st)
    torch.cuda.synchronize()
    sig, osc, eta, tot = [a.cpu().numpy() for a in (sig_d, osc_d, eta_d, tot_d)]
    marked, nm, total = marked_d.cpu().numpy(), int(nm_d.item()), float(sum_d.item())
    assert np.all(sig > 0) and np.all(osc >= 0)
    # the estimator of demo/poisson/demo_error_estimation.py:115-121
    expr = sig + osc + 2 * np.multiply(np.sqrt(sig), np.sqrt(osc))
    assert np.all(np.abs(eta - expr) <= 4 * np.spacing(expr))
    assert abs(tot[2] - np.sum(expr)) <= 1e-13 * np.sum(expr) and abs(total - np.sum(expr)) <= 1e-13 * np.sum(expr)
    assert abs(tot[0] - np.sum(sig)) <= 1e-13 * np.sum(sig) and abs(tot[1] - np.sum(osc)) <= 1e-13 * np.sum(osc)
    # the marked list is the host model's on the downloaded indicators
    order = np.argsort(-eta, kind="stable")
    ref, margin = model_with_margin(eta, order, np.cumsum(eta[order]), theta)
    print(f"  {nm} of {nc} cells marked, margin {margin:.3e}, eta = {np.sqrt(total):.6e}")
    assert margin >= MARGIN
    assert np.array_equal(ref, doerfler_marking(eta, theta))
    assert 0 < nm < nc and nm == ref.size and np.array_equal(marked[:nm], ref) and np.all(marked[nm:] == SENTINEL)
