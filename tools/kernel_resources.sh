#!/bin/bash
# Dev tool: VGPRs / scratch / LDS / occupancy of every kernel in one or more .hip files (hipcc -Rpass-analysis=kernel-resource-usage)
#   tools/kernel_resources.sh latok_amd/csrc/*.hip [extra flags]       all kernels of the library, one sorted list
files=(); flags=()
for a in "$@"; do case $a in *.hip) files+=("$a");; *) flags+=("$a");; esac; done
for f in "${files[@]}"; do
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-function "${flags[@]}" -c "$f" -o /dev/null -Rpass-analysis=kernel-resource-usage 2>&1
done |
  sed 's/ \[-Rpass.*//' |
  awk '/Function Name:/ {n=$NF} / VGPRs:/ {v=$NF} /ScratchSize/ {s=$NF} /Occupancy/ {o=$NF} /LDS Size/ {l=$NF; printf "%s VGPR %s scratch %s occ %s LDS %s\n", n, v, s, o, l}' | c++filt | sed 's/latok:://; s/(latok::[A-Za-z]*)//' | sort
