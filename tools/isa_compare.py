#!/usr/bin/env python3
"""isa_compare.py [REV]: is the gfx950 device code of the work tree that of REV (default HEAD)?

The check of a refactor that must not change code generation.  Every unit of the Makefile's SRCS
is compiled twice with the Makefile's flags plus --cuda-device-only: the work tree's copy, and
REV's copy written to a temporary directory with `git show` (as tools/build_head.sh does, with
the generated eqlb_tables_build_gen.h).  The gfx950 code object is unbundled, disassembled
(llvm-objdump -d) and its notes read (llvm-readelf --notes).  The comparison is per symbol, not
per file offset, since the emission order inside a unit may change: the instruction text without
address and encoding (and without the "..." of the padding up to the next symbol), and per kernel the VGPR/AGPR/SGPR counts, private and group segment size,
kernarg size and maximum workgroup size.  One summary line per unit; kernels present on one side
only and kernels that differ are listed, and any of them makes the exit status 1.  Units without
device code are skipped.  It only diffs two builds against each other.

  --units a.hip b.hip   only these units
  --rename OLD=NEW      a kernel of REV that has another symbol in the tree (one that became a template, say): compared
                        under the new name.  Substrings of the mangled names; each must match one symbol
  --ignore-pcrel        the literal of the s_add_u32 behind an s_getpc_b64 (the distance from the code to a constant
                        table, which moves when the unit's symbols are emitted in another order) is not compared
  --cache DIR           keep REV's side there (by commit hash) for the next call
At most 8 compile jobs run at a time.
"""

import argparse
import concurrent.futures
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "dolfinx_eqlb_amd/csrc"
LLVM = os.environ.get("EQLB_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size",
        ".group_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size")


def sh(*cmd, cwd=ROOT):
    return subprocess.run(cmd, cwd=cwd, check=True, capture_output=True, text=True).stdout


def make_var(csrc_dir, target):
    return sh("make", "-s", "-C", csrc_dir, target).split()


def export_rev(rev, dst):
    """csrc/ and include/ of REV under dst, with the tables that revision's Makefile generates"""
    os.makedirs(os.path.join(dst, CSRC))
    os.makedirs(os.path.join(dst, "include"))
    for f in sh("git", "ls-tree", "--name-only", rev, CSRC + "/", "include/").split():
        with open(os.path.join(dst, f), "wb") as out:
            out.write(subprocess.run(["git", "show", f"{rev}:{f}"], cwd=ROOT, check=True,
                                     capture_output=True).stdout)
    if os.path.exists(os.path.join(dst, CSRC, "eqlb_se_kernels_lowdeg_k4.hip")):
        sh(sys.executable, "tools/gen_tables.py", "--build",
           os.path.join(dst, CSRC, "eqlb_tables_build_gen.h"))


def functions_of(disasm, ignore_pcrel=False):
    """symbol -> instruction lines, without the address and encoding comment"""
    funcs, cur = {}, None
    for line in disasm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
        elif cur is not None and line.startswith(("\t", " ")):
            text = line.split("//")[0].strip()
            if text and text != "...":  # ("...": zero padding up to the next symbol, which moves with the order)
                if ignore_pcrel and cur and cur[-1].startswith("s_getpc_b64") and text.startswith("s_add_u32"):
                    text = re.sub(r"0x[0-9a-f]+$", "<pcrel>", text)
                cur.append(text)
    return funcs


def kernels_of(notes):
    """kernel symbol -> the metadata fields of META"""
    kernels, cur = {}, {}

    def flush():
        if ".symbol" in cur:
            name = cur.pop(".symbol")
            kernels[name] = dict(cur)
        cur.clear()

    for line in notes.splitlines():
        m = re.match(r"^\s*(?:- )?(\.\w+):\s*(\S+)\s*$", line)
        if not m or m.group(1) not in META + (".symbol",):
            continue
        if m.group(1) in cur:  # a key seen twice: the next kernel's record has begun
            flush()
        cur[m.group(1)] = m.group(2).strip("'\"")
    flush()
    return {k[:-3] if k.endswith(".kd") else k: v for k, v in kernels.items()}


def device_code(src, flags, work, ignore_pcrel=False):
    """{'funcs': ..., 'meta': ...} of one unit, or None if it has no device code"""
    stem = os.path.join(work, os.path.basename(src)[:-4])
    sh("/opt/rocm/bin/hipcc", *flags, "--cuda-device-only", "-c", src, "-o", stem + ".bundle")
    sh(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
       "--targets=" + TARGET, "--input=" + stem + ".bundle", "--output=" + stem + ".co")
    if os.path.getsize(stem + ".co") == 0:
        return None
    funcs = functions_of(sh(os.path.join(LLVM, "llvm-objdump"), "-d", stem + ".co"), ignore_pcrel)
    meta = kernels_of(sh(os.path.join(LLVM, "llvm-readelf"), "--notes", stem + ".co"))
    return {"funcs": funcs, "meta": meta} if funcs or meta else None


def renamed(side, renames):
    """REV's side with the symbols of --rename under their names in the tree"""
    for old, new in renames:
        for part in ("funcs", "meta"):
            hits = [n for n in side[part] if old in n and new not in n]
            if len(hits) == 1:
                side[part][hits[0].replace(old, new)] = side[part].pop(hits[0])
    return side


def compare(unit, old, new, renames=()):
    """summary line and findings of one unit"""
    if old is None and new is None:
        return None, []
    old = renamed(old, renames) if old else {"funcs": {}, "meta": {}}
    new = new or {"funcs": {}, "meta": {}}
    names_old = set(old["funcs"]) | set(old["meta"])
    names_new = set(new["funcs"]) | set(new["meta"])
    only_old, only_new = sorted(names_old - names_new), sorted(names_new - names_old)
    findings = [f"  only in REV:  {n}" for n in only_old] + [f"  only in tree: {n}" for n in only_new]
    differ = 0
    for n in sorted(names_old & names_new):
        why = []
        a, b = old["funcs"].get(n, []), new["funcs"].get(n, [])
        if a != b:
            first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            why.append(f"instructions ({len(a)} -> {len(b)}, first difference at {first})")
        ma, mb = old["meta"].get(n, {}), new["meta"].get(n, {})
        why += [f"{k} {ma.get(k)} -> {mb.get(k)}" for k in META if ma.get(k) != mb.get(k)]
        if why:
            differ += 1
            findings.append(f"  differs: {n}: " + "; ".join(why))
    line = (f"{unit}: {len(names_new & set(new['meta']))} kernels, {len(names_new)} symbols, "
            f"{len(only_old)} only in REV, {len(only_new)} only in tree, {differ} differ")
    return line, findings


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("rev", nargs="?", default="HEAD")
    ap.add_argument("--units", nargs="+")
    ap.add_argument("--cache")
    ap.add_argument("--rename", nargs="+", default=[], metavar="OLD=NEW")
    ap.add_argument("--ignore-pcrel", action="store_true")
    args = ap.parse_args()
    sha = sh("git", "rev-parse", args.rev + "^{commit}").strip()
    tmp = tempfile.mkdtemp(prefix="eqlb_isa.")
    try:
        export_rev(sha, os.path.join(tmp, "rev"))
        sh("make", "-s", "-C", os.path.join(ROOT, CSRC), "eqlb_tables_build_gen.h")
        sides = {"rev": os.path.join(tmp, "rev", CSRC), "tree": os.path.join(ROOT, CSRC)}
        flags = make_var(sides["tree"], "print-flags")
        units = {s: make_var(d, "print-srcs") for s, d in sides.items()}
        todo = args.units or sorted(set(units["rev"]) | set(units["tree"]))
        cache = os.path.join(args.cache, sha + ("-nopcrel" if args.ignore_pcrel else "")) if args.cache else None
        result = {"rev": {}, "tree": {}}
        jobs = {}
        with concurrent.futures.ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:
            for side, d in sides.items():
                os.makedirs(os.path.join(tmp, "out_" + side))
                for u in todo:
                    cached = os.path.join(cache, u + ".json") if cache and side == "rev" else None
                    if u not in units[side]:
                        result[side][u] = None
                    elif cached and os.path.exists(cached):
                        result[side][u] = json.load(open(cached))
                    else:
                        jobs[pool.submit(device_code, os.path.join(d, u), flags, os.path.join(tmp, "out_" + side),
                                         args.ignore_pcrel)] = (side, u, cached)
            for fut in concurrent.futures.as_completed(jobs):
                side, u, cached = jobs[fut]
                result[side][u] = fut.result()
                if cached:
                    os.makedirs(os.path.dirname(cached), exist_ok=True)
                    json.dump(result[side][u], open(cached, "w"))
    except subprocess.CalledProcessError as e:
        sys.exit(f"{' '.join(e.cmd)}\n{e.stderr}")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    bad = 0
    for u in todo:
        line, findings = compare(u, result["rev"][u], result["tree"][u], [r.split("=", 1) for r in args.rename])
        if line is None:
            print(f"{u}: no device code, skipped")
            continue
        print(line)
        print("\n".join(findings), end="\n" if findings else "")
        bad += len(findings)
    print(f"isa_compare against {sha[:12]}: " + ("identical" if not bad else f"{bad} findings"))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
