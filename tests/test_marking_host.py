"""The numpy statement of the marking step (dolfinx_eqlb_amd/eqlb/marking.py) - the host model of
tests/test_gpu_marking.py - against the reference's loop restated step by step
(demo/poisson_adaptive/demo_lshape.py:216-242), the tie rule on hand-made arrays, and the combination rule of
indicator_total against the expression of demo/poisson/demo_error_estimation.py:115-121."""

import numpy as np
import pytest

from dolfinx_eqlb_amd.eqlb import doerfler_marking
from dolfinx_eqlb_amd.eqlb.marking import indicator_total


def reference_loop(eta, theta):
    """The steps of the reference's marking, one by one: argsort, reversed; a Python loop over the running sum that
    stops at the first value strictly above the cut-off; np.sort of the cells up to there (all, if it never stops)."""
    if np.isclose(theta, 1.0):
        return np.arange(eta.size, dtype=np.int32)
    limit = theta * np.sum(eta)
    descending = np.argsort(eta)[::-1]
    acc, stop = 0.0, eta.size
    for pos, cell in enumerate(descending):
        acc += eta[cell]
        if acc > limit:
            stop = pos
            break
    return np.sort(descending[:stop + 1]).astype(np.int32)


@pytest.mark.parametrize("ncells", [1, 2, 3, 64, 257, 4097])
@pytest.mark.parametrize("theta", [0.01, 0.3, 0.5, 0.6, 0.9, 0.999, 1.0 - 1e-9, 1.0])
def test_model_is_the_reference_loop_on_tie_free_input(ncells, theta):
    for s in range(3):
        eta = np.random.default_rng(20241003 + s).lognormal(0, 2, ncells)
        assert np.unique(eta).size == ncells
        got = doerfler_marking(eta, theta)
        assert got.dtype == np.int32 and np.array_equal(got, reference_loop(eta, theta))


def test_tie_rule_equal_values_in_ascending_cell_id():
    # all equal: the first cells; 257 * 0.5 = 128.5 is exceeded by 129 cells
    assert np.array_equal(doerfler_marking(np.ones(257), 0.5), np.arange(129))
    # 8 > 2 = 2 = 2 > 1: cut-off 0.7 * 15 = 10.5 -> 8, then the twos of the LOWEST ids (cells 0 and 3)
    eta = np.array([2.0, 1.0, 8.0, 2.0, 2.0])
    assert np.array_equal(doerfler_marking(eta, 0.7), [0, 2, 3])
    assert np.array_equal(doerfler_marking(eta, 0.5), [2])      # 8 > 7.5
    assert np.array_equal(doerfler_marking(eta, 0.6), [0, 2])   # 8 + 2 > 9
    assert np.array_equal(doerfler_marking(eta, 0.9), [0, 2, 3, 4])  # 14 > 13.5
    # ties below the threshold value do not matter, ties above it are all in
    eta = np.array([1.0, 4.0, 4.0, 1.0, 3.0])
    assert np.array_equal(doerfler_marking(eta, 0.7), [1, 2, 4])  # 11 > 9.1
    # -0.0 is a zero
    assert np.array_equal(doerfler_marking(np.array([-0.0, 0.0, 1.0]), 0.5), [2])


def test_edge_cases():
    assert np.array_equal(doerfler_marking(np.zeros(7), 0.5), np.arange(7))  # no prefix exceeds 0
    eta = np.full(100, 1e-3)
    eta[41] = 1.0
    assert np.array_equal(doerfler_marking(eta, 0.5), [41])
    assert np.array_equal(doerfler_marking([3.0], 0.2), [0])
    for theta in (1.0, 1.0 - 1e-9, 1.0 + 1e-9):
        assert np.array_equal(doerfler_marking(np.arange(5.0), theta), np.arange(5))
    for theta in (0.0, -0.5, 1.1, float("nan")):
        with pytest.raises(ValueError, match="theta"):
            doerfler_marking(np.ones(4), theta)
    with pytest.raises(ValueError, match="no cells"):
        doerfler_marking(np.zeros(0), 0.5)
    with pytest.raises(ValueError, match="cell 2"):
        doerfler_marking(np.array([1.0, 0.0, float("nan"), -1.0]), 0.5)
    with pytest.raises(ValueError, match="cell 1"):
        doerfler_marking(np.array([1.0, -1e-300, 2.0]), 0.5)


@pytest.mark.parametrize("nterms", [1, 2, 3, 4])
def test_indicator_total_combination_rule(nterms):
    rng = np.random.default_rng(5 + nterms)
    terms = rng.lognormal(0, 2, (nterms, 1001))
    eta2, totals = indicator_total(terms)
    assert np.allclose(eta2, terms.sum(axis=0), rtol=1e-15, atol=0)
    assert np.allclose(totals, list(terms.sum(axis=1)) + [eta2.sum()], rtol=1e-14, atol=0)
    if nterms < 2:
        with pytest.raises(ValueError):
            indicator_total(terms, pair_last_two=True)
        return
    eta2, totals = indicator_total(terms, pair_last_two=True)
    Leta_sig, Leta_osc = terms[-2], terms[-1]
    ref = Leta_sig + Leta_osc + 2 * np.multiply(np.sqrt(Leta_sig), np.sqrt(Leta_osc))  # demo_error_estimation.py:117-119
    if nterms == 2:
        assert np.array_equal(eta2, ref)
    assert np.allclose(eta2, terms[:-2].sum(axis=0) + ref, rtol=4e-16, atol=0)
    assert np.allclose(eta2, terms[:-2].sum(axis=0) + (np.sqrt(Leta_sig) + np.sqrt(Leta_osc)) ** 2, rtol=1e-15, atol=0)
    assert abs(totals[-1] - np.sum(eta2)) <= 1e-14 * totals[-1]
    assert np.allclose(totals[:-1], terms.sum(axis=1), rtol=1e-14, atol=0)


def test_symbols_are_declared_for_the_abi_test():
    from dolfinx_eqlb_amd import cpp
    for s in ("eqlb_indicator_total", "eqlb_mark_doerfler"):
        assert s in cpp.EXPORTED_SYMBOLS
    for name in ("indicator_total", "indicator_total_raw", "mark_doerfler", "mark_doerfler_raw"):
        assert callable(getattr(cpp, name))
