"""The reference tensors compiled into the library for every (k, degree of the projected data) pair the device runs,
1 <= k <= 4, 0 <= d <= k-1, are the generated ones (host entry point, no GPU)."""

import numpy as np
import pytest

PAIRS = [(k, d) for k in range(1, 5) for d in range(k)]


@pytest.mark.parametrize("k,deg", PAIRS)
def test_reference_tables_match_generator(k, deg):
    from dolfinx_eqlb_amd import cpp
    from gen_tables import tables_float
    t = tables_float(k, deg)
    for name in "SFHD":
        assert np.array_equal(cpp.get_reference_table(k, deg, name), t[name]), name


def test_generator_lists_every_pair():
    from gen_tables import PAIRS as GEN, PAIRS_BUILD
    assert sorted(GEN + PAIRS_BUILD) == sorted(PAIRS)
