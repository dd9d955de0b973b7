#!/bin/bash
# build_variant.sh NAME "-DFOO=1 -DBAR=2": timing-experiment build of libeqlb_amd.so into build_exp/lib_NAME.so with other
# values of the build parameters (csrc/eqlb_tuning.h)
# (only eqlb_se_kernels.hip is recompiled; run with EQLB_AMD_LIB=build_exp/lib_NAME.so python bench.py)
set -e
cd "$(dirname "$0")/.."
mkdir -p build_exp
SRC=dolfinx_eqlb_amd/csrc
FILE=${3:-eqlb_se_kernels}
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function $2 -c $SRC/$FILE.hip -o build_exp/${FILE}_$1.o
OBJS=""
# (the objects of the library: the Makefile's list)
for f in $(make -s -C $SRC print-srcs | sed 's/\.hip//g'); do
  if [ "$f" = "$FILE" ]; then OBJS="$OBJS build_exp/${FILE}_$1.o"; else OBJS="$OBJS $SRC/$f.o"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o build_exp/lib_$1.so $OBJS -ldl
echo built build_exp/lib_$1.so
