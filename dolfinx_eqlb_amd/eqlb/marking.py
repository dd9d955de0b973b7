"""Cell-wise indicator and Doerfler marking: the numpy statement of what eqlb_indicator_total and
eqlb_mark_doerfler (include/eqlb.h) compute on the device.

This is documentation and the host model of the tests, not a fallback: the product path is
dolfinx_eqlb_amd.cpp.indicator_total / mark_doerfler.  The rule is the one of the reference's adaptive demos
(demo/poisson_adaptive/demo_lshape.py:216-242): order the cells by descending indicator, mark the shortest
prefix whose running sum is strictly greater than theta * total, return the marked ids sorted.  Where the
reference leaves the order among equal values to np.argsort, equal values are taken in ascending cell id here.
"""

import numpy as np

__all__ = ("indicator_total", "doerfler_marking")


def indicator_total(terms, pair_last_two=False):
    """(cell_eta2 [ncells], totals [nterms + 1]) of squared cell-wise terms [nterms, ncells].

    cell_eta2 is the sum of the terms; with pair_last_two the last two, a and b, enter as
    (sqrt a + sqrt b)^2 = a + b + 2 sqrt(a) sqrt(b) - Leta_sig + Leta_osc + 2 sqrt(Leta_sig) sqrt(Leta_osc) of
    demo/poisson/demo_error_estimation.py:115-121.  totals: the sum over the cells of every term, then of cell_eta2.
    """
    t = [np.ascontiguousarray(v, dtype=np.float64).ravel() for v in terms]
    if not 1 <= len(t) <= 8 or (pair_last_two and len(t) < 2) or any(v.size != t[0].size for v in t):
        raise ValueError("indicator_total: 1 ... 8 terms of one length (at least 2 with pair_last_two)")
    plain = t[:-2] if pair_last_two else t
    eta2 = np.zeros_like(t[0])
    for v in plain:
        eta2 = eta2 + v
    if pair_last_two:
        a, b = t[-2], t[-1]
        eta2 = eta2 + a + b + 2 * np.multiply(np.sqrt(a), np.sqrt(b))
    return eta2, np.array([np.sum(v) for v in t] + [np.sum(eta2)])


def doerfler_marking(cell_eta2, theta):
    """Sorted int32 ids of the cells Doerfler marking with parameter theta selects.

    cell_eta2 [ncells] non-negative.  |theta - 1| <= 1e-8 (np.isclose(theta, 1.0) of the reference) marks every
    cell, and so does a cut-off that no prefix exceeds (all indicators zero).  Equal values: ascending cell id.
    """
    eta = np.ascontiguousarray(cell_eta2, dtype=np.float64).ravel()
    n = eta.size
    if n < 1:
        raise ValueError("doerfler_marking: no cells")
    if not (theta > 0.0 and theta <= 1.0 + 1e-8):
        raise ValueError(f"doerfler_marking: theta = {theta} outside (0, 1]")
    bad = np.flatnonzero(~(eta >= 0.0))
    if bad.size:
        raise ValueError(f"doerfler_marking: negative or NaN indicator in cell {bad[0]}")
    if abs(theta - 1.0) <= 1e-8:
        return np.arange(n, dtype=np.int32)
    cutoff = theta * np.sum(eta)
    # descending value, equal values in ascending cell id: a stable sort of the negated values
    order = np.argsort(-eta, kind="stable")
    running = np.cumsum(eta[order])  # sequential, as the reference's loop
    over = np.flatnonzero(running > cutoff)
    nmarked = int(over[0]) + 1 if over.size else n
    return np.sort(order[:nmarked]).astype(np.int32)
