#!/bin/bash
# bash scripts/regs.sh <file.hip> [name filter] [extra hipcc flags]: register / scratch / occupancy report per kernel
f=$1; filt=${2:-.}; shift; shift
cd $(dirname $f)
# (the unit's own flags, as the Makefile beside it has them, before the extra ones)
unit=$(make -s --no-print-directory unit-flags-$(basename ${f%.hip}) 2>/dev/null)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -munsafe-fp-atomics -fno-hip-fp32-correctly-rounded-divide-sqrt \
  -Rpass-analysis=kernel-resource-usage $unit "$@" -c $(basename $f) -o /tmp/regs.o 2>&1 |
  awk '/Function Name/{name=$0; sub(/.*Function Name: /,"",name); sub(/ \[.*/,"",name)} /VGPRs:|AGPRs:|ScratchSize|Occupancy|VGPRs Spill|SGPRs Spill/{v=$0; sub(/.*remark: +/,"",v); sub(/ \[-Rpass.*/,"",v); out[name]=out[name] " | " v} END{for(n in out) print n out[n]}' | grep -E "$filt" | sed 's/_ZN4gvpm//'
