"""The integer rules that the three weak-symmetry kernels share (csrc/eqlb_se_weaksym_numbering.h), checked on the host
by a program of its own."""

import os
import shutil
import subprocess

import pytest


def test_numbering_stand_alone_under_sanitizers(tmp_path):
    """tools/weaksym_numbering_check.cpp under AddressSanitizer and UBSan where the compiler has them: for K = 2, 3, 4,
    interior and boundary patches of 2 ... 64 cells (the chain also 65, 200 and 1000) and the 16 combinations of the
    flux-BC flags of the two stress rows, the dense and the chain numbering cover 0 ... dim - 1, neighbours agree on
    their facet, the points of the multipliers lie in 0 ... npnt - 1 with the node at 0 and a shared ring point between
    consecutive cells, the chain entries of a cell lie within the half bandwidth or in the border, bslot is 0 exactly
    for the node, and fixed marks d, facet 0 and the last facet by the row's flags."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "weaksym_numbering_check")
    base = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
            os.path.join(root, "tools", "weaksym_numbering_check.cpp"), "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True,
                         text=True)
    if san.returncode != 0:   # (a compiler without the sanitizer runtimes: the rules are still checked)
        subprocess.run(base, check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    # 3 degrees x (63 + 3 sizes) x interior / boundary x 16 flag combinations
    assert run.stdout.splitlines()[-1] == f"checked {3 * 66 * 2 * 16} patches"
