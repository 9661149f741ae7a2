#!/bin/bash
# bash scripts/build_variant.sh NAME FILE.hip "<extra hipcc flags>": an A/B copy of libgvpm_hip.so with ONE translation unit
# rebuilt with extra flags -> build/variants/libgvpm_hip_NAME.so (run with GVPM_HIP_LIB=<that path>; probes only)
set -e
name=$1; file=$2; shift; shift
root=$(cd "$(dirname "$0")/.." && pwd)
cs=$root/gvpm_amd/csrc
out=$root/build/variants
mkdir -p $out
make -s -C $cs
obj=$out/${file%.hip}_$name.o
# (the unit's own flags, as the Makefile has them, come before the variant's: a later -fslp-vectorize overrides an earlier -fno-)
unit=$(make -s --no-print-directory -C $cs unit-flags-${file%.hip})
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -munsafe-fp-atomics -fno-hip-fp32-correctly-rounded-divide-sqrt \
  -Wno-unused-function -Wno-unused-variable -Wno-unused-result $unit "$@" -I$cs -c $cs/$file -o $obj
# the library's objects as the Makefile lists them, the one of FILE.hip replaced
objs=""
for o in $(make -s --no-print-directory -C $cs print-objs); do
  if [ "$o" == "${file%.hip}.o" ]; then objs="$objs $obj"; else objs="$objs $cs/$o"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $out/libgvpm_hip_$name.so $objs -ldl
echo $out/libgvpm_hip_$name.so
