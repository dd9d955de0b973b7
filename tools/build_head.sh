#!/bin/bash
# build_head.sh [REV]: complete libeqlb_amd.so of a committed revision (default HEAD) into
# build_exp/lib_head.so, for same-call A/B runs (tools/run_variants.sh).  ALL objects come from that
# revision: mixing objects of two revisions breaks as soon as a struct shared by host and device
# code changes (a mismatched TileDesc made the kernel read out of bounds).
set -e
cd "$(dirname "$0")/.."
REV=${1:-HEAD}
T=$(mktemp -d /tmp/eqlb_head.XXXXXX)
mkdir -p "$T/dolfinx_eqlb_amd/csrc" "$T/include" build_exp
for f in $(git ls-tree --name-only "$REV" dolfinx_eqlb_amd/csrc/ include/); do
  git show "$REV:$f" > "$T/$f"
done
# tables that revision's Makefile generates instead of keeping them in git (tools/gen_tables.py --build)
if [ -f "$T/dolfinx_eqlb_amd/csrc/eqlb_se_kernels_lowdeg_k4.hip" ]; then
  python3 tools/gen_tables.py --build "$T/dolfinx_eqlb_amd/csrc/eqlb_tables_build_gen.h"
fi
OBJS=""
# every translation unit of that revision, in the link order of its Makefile: units share weak host stubs of rocPRIM
# kernels (eqlb_tiling_device.o and eqlb_mesh_build.o: 169), the linker keeps those of the first object, and the code
# object that a launch loads is that object's - in alphabetical order the tiler's sorts loaded the 11 ms code object
# of eqlb_mesh_build inside the first set_boundary instead of the one device_tiling_prepare() had loaded
UNITS=$(make -s -C "$T/dolfinx_eqlb_amd/csrc" print-srcs 2>/dev/null | sed 's/\.hip//g')
[ -n "$UNITS" ] || UNITS=$(git ls-tree --name-only "$REV" dolfinx_eqlb_amd/csrc/ | grep '\.hip$' | xargs -n1 basename | sed 's/\.hip$//')
for f in $UNITS; do
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-function -c "$T/dolfinx_eqlb_amd/csrc/$f.hip" -o "$T/$f.o" &
  OBJS="$OBJS $T/$f.o"
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o build_exp/lib_head.so $OBJS
rm -rf "$T"
echo built build_exp/lib_head.so from $REV
