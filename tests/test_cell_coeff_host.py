"""The admission rules of the cell-wise coefficients (csrc/eqlb_cell_coeff.h), checked on the host by a program of its
own: predicates, the first bad cell of an array and the messages, against the lines written out here."""

import os
import shutil
import subprocess

import pytest

# -inf, -1, nextafter(-1, 0), -0.0, 0, denorm_min, 1, DBL_MAX, +inf, NaN
EXPECTED = """\
rule non-negative: 0 0 0 1 1 1 1 1 0 0
rule positive: 0 0 0 0 0 1 1 1 0 0
rule above -1: 0 0 1 1 1 1 1 1 1 0
tensor (1, 0, 1): ok
tensor (1, 1, 1): not definite
tensor (0, 0, 1): not definite
tensor (-1, 0, -1): not definite
tensor (1, nan, 1): not finite
tensor (inf, 0, 1): not finite
tensor (nan, 0, -1): not finite
tensor (1e-200, 0, 1e-200): not definite
scan cell_c: -1 0 3 9 -1
scan cell_mu: -1 0 3 9 -1
scan cell_pi1: -1 0 3 9 -1
scan cell_D: -1 0 3 9 -1
eqlb_x: c = -1 is negative, NaN or infinite
eqlb_x: alpha = inf is negative, NaN or infinite
eqlb_x: mu = 0 is zero, negative, NaN or infinite
eqlb_x: cell_c[3] = -0.5 is negative, NaN or infinite
eqlb_x: facet_alpha[0] = -2 is negative, NaN or infinite
eqlb_x: cell_mu[11] = -1 is zero, negative, NaN or infinite
eqlb_x: cell_coeff[2] = 0 is zero, negative, NaN or infinite
eqlb_x: cell_pi1[4] = -1 is not above -1
eqlb_x: cell_D[1] = (1, inf, 1) is not finite
eqlb_x: cell_D[2] = (1, 2, 1) is not positive definite
"""


def test_rules_stand_alone_under_sanitizers(tmp_path):
    """tools/cell_coeff_check.cpp under AddressSanitizer and UBSan where the compiler has them.  The three scalar rules
    on the ten values above (-0.0 is non-negative and not positive; -1 is not above -1, its neighbour towards 0 is, and so
    is +inf); the tensor rule (determinant exactly 0 and a product that underflows to 0 are not definite; "not finite"
    comes before "not definite"); the first bad cell of an array per rule - no entry (nothing is read: a null pointer),
    one bad entry, bad entries 3 and 7, the last entry alone, none; and one message of each form, as the formats
    "%s: c = %g ...", "%s: cell_c[%lld] = %g ..." and "%s: cell_D[%lld] = (%g, %g, %g) ..." print them."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "cell_coeff_check")
    base = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
            os.path.join(root, "tools", "cell_coeff_check.cpp"), "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True,
                         text=True)
    if san.returncode != 0:   # (a compiler without the sanitizer runtimes: the rules are still checked)
        subprocess.run(base, check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.splitlines() == EXPECTED.splitlines()
