#!/usr/bin/env python3
"""record_primal_bits.py [--out FILE]: writes tests/golden/primal_solve_bits.json, the recording that
tests/test_gpu_primal_solve_bits.py pins the P_p solves to.

Needs the device.  The cases, and what is kept of a solve, are those of the test module (compute, CASES); everything
runs through the public Python API, so the library that EQLB_AMD_LIB names serves as well as the one in the tree:

    tools/build_head.sh REV && EQLB_AMD_LIB=build_exp/lib_head.so python tools/record_primal_bits.py

records the bits of revision REV.  Regenerate only for a change that means to alter the order of a sum or a rule of
the iteration (the docstring of the test module)."""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "primal_solve_bits.json"))
    args = ap.parse_args()
    import torch
    torch.cuda.init()   # (torch's HIP runtime first, as tests/conftest.py does)
    import test_gpu_primal_solve_bits as tb
    from dolfinx_eqlb_amd import cpp
    cases = {}
    for name in tb.CASES:
        cases[name] = tb.compute(name)
        print(f"{name}: " + ", ".join(f"{entry} {len(cols)} column(s)" for entry, cols in cases[name].items()),
              flush=True)
    with open(args.out, "w") as f:
        json.dump(dict(library=os.path.basename(cpp.LIB_PATH), info_keys=list(tb.INFO_KEYS), cases=cases), f, indent=1,
                  sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
