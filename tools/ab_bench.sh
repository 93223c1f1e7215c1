#!/bin/bash
# A/B of two builds of libmirhi.so on ONE box, interleaved (boxes differ by +-10 %): tools/ab_bench.sh libA.so libB.so [rounds] [bench args...]
# prints value (Mtris/s), raster / geometry kernel us (isolated), us per frame
# A or B may also be a DIRECTORY: another built checkout, whose own bench.py and package run its libmirhi.so -- for a build whose C ABI differs
# (a function the other build's library lacks: the Python binding resolves every declared symbol, so one tree cannot load both libraries)
A=$1; B=$2; R=${3:-3}; shift 3
HERE=$(pwd)
for r in $(seq 1 $R); do
  for L in $A $B; do
    if [ -d "$L" ]; then cd "$L"; unset MIRHI_LIB_NAME; else cd "$HERE"; export MIRHI_LIB_NAME=$L; fi
    python bench.py --full --no-cpu-baseline --no-extras "$@" 2>/dev/null | python -c "
import json,sys
j=json.loads(sys.stdin.readline()); rf=j['roofline']
print('$L', 'round $r', 'value', j['value'], 'us/frame', j['us_per_frame'], 'raster', rf['avg_kernel_us'], 'geometry', rf['geometry_kernel_us'], 'vertex', rf['vertex_kernel_us'])"
    cd "$HERE"; unset MIRHI_LIB_NAME
  done
done
