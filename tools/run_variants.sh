#!/bin/bash
# run_variants.sh "bench args" NAME...: bench.py once per timing-experiment library (on the GPU box)
ARGS="$1"; shift
# (--full: the per-kernel times printed below; logs under $OUT)
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
for v in "$@"; do
  if [ "$v" = "base" ]; then L=dolfinx_eqlb_amd/libeqlb_amd.so; else L=build_exp/lib_$v.so; fi
  EQLB_AMD_LIB=$L python bench.py --full --no-cpu-baseline $ARGS > "$OUT/var_$v.log" 2>&1 || { echo "$v FAILED"; tail -3 "$OUT/var_$v.log"; exit 1; }
  python - "$v" "$OUT/var_$v.log" <<'PY'
import json, sys
v = sys.argv[1]
d = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
print(f"{v:16s} ms/step {d['ms_per_step']:.4f}  kernels {d['roofline'].get('all_kernels_ms')}")
PY
done
