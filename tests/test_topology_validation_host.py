"""Which nodes the patch builder can walk and which facet-type tables eqlb_se_set_boundary refuses, on the host (no
GPU): tools/topology_check_emul.cpp includes dolfinx_eqlb_amd/csrc/eqlb_topology_check.h - the header the library's
own checks come from - and feeds it small meshes written down there: a 2 x 2 crossed square, a crossed square with a
hole, a bow-tie of two pairs of triangles, a node of one cell, a boundary loop with an untyped facet, a typed facet
between two cells, on the first and on the second row of the table, and node masks that hide each offender (or only one
of its nodes).  The program checks the verdict and the named node / facet of every table; it is built as a plain
executable with the address and undefined-behaviour sanitizers where the compiler has them."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_topology_check_emulation(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src = os.path.join(ROOT, "tools", "topology_check_emul.cpp")
    exe = str(tmp_path / "topology_check_emul")
    base = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", src, "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True,
                         text=True)
    if san.returncode != 0:   # (a compiler without the sanitizer runtimes: the tables are still checked)
        subprocess.run(base, check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.strip().endswith("PASS")
