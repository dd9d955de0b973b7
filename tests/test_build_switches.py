"""Source lint of dolfinx_eqlb_amd/csrc: no file includes a .hip, and the EQLB_* names a -D on the
compiler's command line can override are exactly those declared in eqlb_tuning.h (numeric
parameters of size, occupancy and tolerance; decided code variants are resolved in the source,
DESIGN.md "retired build switches").  Device memory has one home: only eqlb_host_util.h names the
allocator and the calls that create or destroy an event or a stream, and the hand-rolled stagings, frees and
first-use uploads it replaced stay away."""

import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dolfinx_eqlb_amd", "csrc")
TUNING = "eqlb_tuning.h"

# Names that the rules below find but that are no build parameters:
#   include guards: none in csrc (its headers use #pragma once)
#   function-like helper macros: defined unconditionally, so the rules do not find them
#   the platform test of eqlb_pair_chain.h, which the host emulation (tools/pair_chain_emul.cpp) includes too:
#   its function qualifier is defined under "#ifndef EQLB_PC_FN"
EXCLUDED = {"EQLB_PC_FN"}


def _sources():
    # (eqlb_tables_build_gen.h: written by the build, literals only)
    files = [f for f in glob.glob(os.path.join(CSRC, "*")) if f.endswith((".hip", ".h", ".cpp", ".hpp"))]
    assert len(files) > 30
    return {os.path.basename(f): open(f).read() for f in sorted(files)}


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _directives(text):
    """(directive, rest) of every preprocessor line, continuation lines joined"""
    text = _strip_comments(text).replace("\\\n", " ")
    return re.findall(r"^[ \t]*#[ \t]*(\w+)\b[ \t]*(.*)$", text, flags=re.M)


def _overridable(text):
    """EQLB_* names tested by #if / #ifdef / #ifndef / #elif / defined(), or #defined under an #ifndef of themselves"""
    names, guard = set(), []
    for d, rest in _directives(text):
        if d in ("if", "ifdef", "ifndef", "elif"):
            names |= set(re.findall(r"\bEQLB_\w+", rest))
        if d in ("if", "ifdef", "ifndef"):
            guard.append(rest.split()[0] if d == "ifndef" and rest.split() else None)
        elif d == "endif":
            guard.pop()
        elif d == "define":
            m = re.match(r"(EQLB_\w+)", rest)
            if m and m.group(1) in guard:
                names.add(m.group(1))
    return names


def _defined(text):
    return {m.group(1) for d, rest in _directives(text) if d == "define" for m in [re.match(r"(EQLB_\w+)", rest)] if m}


def test_no_file_includes_a_hip():
    for name, text in _sources().items():
        for d, rest in _directives(text):
            assert not (d == "include" and ".hip" in rest), f"{name}: #include {rest}"


def test_overridable_names_are_those_of_the_tuning_header():
    src = _sources()
    declared = _overridable(src[TUNING])
    assert declared and declared == _defined(src[TUNING])
    found = set()
    for text in src.values():
        found |= _overridable(text)
    assert found - EXCLUDED == declared, sorted((found - EXCLUDED) ^ declared)


def test_parameters_are_defined_in_the_tuning_header_only():
    src = _sources()
    declared = _overridable(src[TUNING])
    for name, text in src.items():
        if name != TUNING:
            assert not (_defined(text) & declared), f"{name}: {sorted(_defined(text) & declared)}"


def test_every_parameter_is_used():
    src = _sources()
    used = set()
    for name, text in src.items():
        if name != TUNING:
            used |= set(re.findall(r"\bEQLB_\w+", _strip_comments(text)))
    assert _overridable(src[TUNING]) <= used


def _hip_sources():
    return {name: text for name, text in _sources().items() if name.endswith((".hip", ".h"))}


def test_only_the_host_helpers_name_the_device_allocator():
    # (comments included: a file that speaks of the allocator is about to call it)
    for name, text in _hip_sources().items():
        if name != "eqlb_host_util.h":
            found = sorted(set(re.findall(r"\bhip(?:Malloc|Free|MallocAsync|FreeAsync)\b", text)))
            assert not found, f"{name}: {found}"
    helpers = _hip_sources()["eqlb_host_util.h"]
    for word in ("hipMalloc", "hipFree", "hipMallocAsync", "hipFreeAsync"):
        assert re.search(rf"\b{word}\b", helpers), word


def test_only_the_host_helpers_name_the_event_and_stream_calls():
    # (comments included, as for the allocator)
    calls = r"\bhip(?:EventCreate\w*|EventDestroy|StreamCreate\w*|StreamDestroy)\b"
    for name, text in _hip_sources().items():
        if name != "eqlb_host_util.h":
            found = sorted(set(re.findall(calls, text)))
            assert not found, f"{name}: {found}"
    helpers = _hip_sources()["eqlb_host_util.h"]
    for word in ("hipEventCreateWithFlags", "hipEventDestroy", "hipStreamCreateWithFlags", "hipStreamDestroy"):
        assert re.search(rf"\b{word}\b", helpers), word


def test_no_file_frees_or_uploads_through_a_bare_pointer():
    # the free functions dfree(p) and upload(&p, ...) are gone: DevBuf frees and uploads what it owns
    for name, text in _hip_sources().items():
        if name != "eqlb_host_util.h":
            for gone in (r"\bdfree\s*\(", r"(?<![\w.>])upload\s*(?:<[^>]*>\s*)?\(\s*&"):
                assert not re.search(gone, text), f"{name}: {gone}"


def test_the_mesh_view_holds_no_host_copies():
    text = _strip_comments(_hip_sources()["eqlb_internal.h"])
    body = re.search(r"\bstruct\s+DeviceMesh\s*\{(.*?)\n\};", text, flags=re.S)
    assert body and "nnodes" in body.group(1)
    assert "std::vector" not in body.group(1)
    assert not re.search(r"\bstruct\s+eqlb_mesh\s*\{", text)  # (the owner lives in a host-only header)


def test_node_cells_is_uploaded_in_one_place():
    # the hand-written "upload on first use" test of the table, with any receiver
    for name, text in _hip_sources().items():
        assert not re.search(r"!\s*[\w.>-]*\bnode_cells\s*&&", text), name


def test_the_replaced_stagings_stay_away():
    for name, text in _hip_sources().items():
        for gone in (r"#\s*define\s+fail\b", r"\bstruct\s+Staging\b", r"\bstruct\s+HostStage\b"):
            assert not re.search(gone, text), f"{name}: {gone}"


def test_grid_of_is_defined_once():
    defs = [name for name, text in _hip_sources().items()
            for _ in re.finditer(r"^[ \t]*(?:\w+[ \t]+)+grid_of[ \t]*\([^;{]*\)\s*\{", _strip_comments(text), flags=re.M)]
    assert defs == ["eqlb_host_util.h"], defs
