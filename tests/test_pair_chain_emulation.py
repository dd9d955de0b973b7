"""The lane arithmetic of the RT_2 full-patch body on the host (no GPU): tools/pair_chain_emul.cpp runs the templates
of dolfinx_eqlb_amd/csrc/eqlb_pair_chain.h with the lanes of a patch as array indices - the pair-lane mapping (4 lanes,
two ring cells each) and the lane = cell mapping (8 lanes) on the same random rings of 8 cells - and compares them
with each other, with a dense solve of the reduced system and with a sequential walk round the ring. The bounds are
the program's own (printed with the figures); it is built as a plain executable with the address and
undefined-behaviour sanitizers where the compiler has them.

Its second mode feeds pair_chain rings with a cell of det J = 0: the te / le blocks as phase C builds them (metric
J^T J / |det J| times reference tensors, so inf and NaN entries), the bad cell on each of the eight ring positions, and
a healthy ring with a single +inf that reaches the last pivot only.  `ok` has to come back false for every one of
them (and true on the healthy rings): the pivot test is "positive and finite", a > 0 alone lets the lone +inf through."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src = os.path.join(ROOT, "tools", "pair_chain_emul.cpp")
    exe = str(tmp_path_factory.mktemp("pair_chain") / "pair_chain_emul")
    base = [cxx, "-O1", "-std=c++17", "-Wall", "-Werror", src, "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True,
                         text=True)
    if san.returncode != 0:   # (a compiler without the sanitizer runtimes: the comparison still runs)
        subprocess.run(base, check=True)
    return exe


def test_pair_chain_emulation(emulator):
    run = subprocess.run([emulator, "500"], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.strip().endswith("PASS")


def test_pair_chain_flags_a_flat_cell_on_every_ring_position(emulator):
    run = subprocess.run([emulator, "degenerate", "200"], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.strip().endswith("PASS")
    lines = run.stdout.splitlines()
    assert any(ln.startswith("flat cell: rings 6400") and "pair 0" in ln and "cell 0" in ln for ln in lines)
    assert any(ln.startswith("+inf on the last pivot: rings 400") and "pair 0" in ln for ln in lines)
