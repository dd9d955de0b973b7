"""The table of a facet term - the Robin term of a Poisson handle, the spring term of an elasticity handle
(csrc/eqlb_facet_plan.h) - built on the host by a program of its own, against the lines written out here."""

import os
import shutil
import subprocess

import pytest

# Worked out by hand from the rule in the header: an entry (row, facet, position, local index) per row of a listed facet
# with flag 1, sorted by row, facet, position; ent = position * 8 + local index; chunk[c] = the first row >= c *
# chunk_dofs, the last one m; layout = dofs, chunk, rows, off, ent, total = n, 6 n, + nchunk, + m, + m + 1, + nent.
EXPECTED = """\
case pair p=1
rows: 0 1 2 3
off: 0 2 4 6 8
ent: 0 8 1 16 9 24 17 25
chunk: 0 4
layout: 4 24 26 30 35 43, m 4
case pair p=3
rows: 0 1 2 3 4 5 6 7 10 11 12 13
off: 0 2 4 6 8 9 10 11 12 13 14 15 16
ent: 0 8 1 16 9 24 17 25 2 3 10 11 18 19 26 27
chunk: 0 12
layout: 4 24 26 38 51 67, m 12
case pinch
rows: 0 1 2 3 4
off: 0 4 5 6 7 8
ent: 0 8 16 24 1 9 17 25
chunk: 0 5
layout: 4 24 26 31 37 45, m 5
case descending
rows: 0 1 2 3 4
off: 0 4 5 6 7 8
ent: 24 16 8 0 25 17 9 1
chunk: 0 5
layout: 4 24 26 31 37 45, m 5
case skipped
rows: 1 4 5 8 13
off: 0 1 3 4 5 6
ent: 8 9 24 25 10 26
chunk: 0 5
layout: 5 30 32 37 43 49, m 5
case 512 by 256
rows: 100 255 256 511
off: 0 1 3 5 6
ent: 0 1 8 9 16 17
chunk: 0 2 4
layout: 3 18 21 25 30 36, m 4
case 512 by 128
rows: 100 255 256 511
off: 0 1 3 5 6
ent: 0 1 8 9 16 17
chunk: 0 1 2 3 4
layout: 3 18 23 27 32 38, m 4
case 513 by 256
rows: 100 255 256 511 512
off: 0 1 3 5 7 8
ent: 0 1 8 9 16 17 24 25
chunk: 0 2 4 5
layout: 4 24 28 33 39 47, m 5
case 513 by 128
rows: 100 255 256 511 512
off: 0 1 3 5 7 8
ent: 0 1 8 9 16 17 24 25
chunk: 0 1 2 3 4 5
layout: 4 24 30 35 41 49, m 5
case nothing left
rows:
off: 0
ent:
chunk: 0 0
layout: 2 12 14 14 15 15, m 0
"""


def test_tables_stand_alone_under_sanitizers(tmp_path):
    """tools/facet_plan_check.cpp under AddressSanitizer and UBSan where the compiler has them.  The four boundary
    facets of a triangle pair at p = 1 and p = 3 (a corner row lies in two facets; chunks of 256 and of 128 DOFs); the
    pinch node of a bowtie in four listed facets, and the same list in descending facet id (the entries of a row still
    ascend by facet, the positions in them descend); skipped positions (flag 0 and 2) in front, in the middle and at
    the end; rows on both sides of a chunk boundary with ndofs a multiple of the chunk and one more, for chunks of 256
    and 128 DOFs; a list of which nothing is left."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "facet_plan_check")
    base = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
            os.path.join(root, "tools", "facet_plan_check.cpp"), "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True,
                         text=True)
    if san.returncode != 0:   # (a compiler without the sanitizer runtimes: the tables are still checked)
        subprocess.run(base, check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.splitlines() == EXPECTED.splitlines()
