#!/bin/bash
# A/B of builds of libmirhi.so on ONE box, interleaved, natively dispatched, with the frame-loop extras: tools/ab_full.sh "libA.so libB.so ..." [rounds] [bench args...]
# (variants: python renderer-rs_amd/build.py --variant NAME -DX=1 -> libmirhi_NAME.so + its code object)
# The order of the libraries rotates by one from round to round.  Every bench runs under its own time limit (MIRHI_AB_LIMIT seconds, default 150), and the first
# one that fails ends the comparison: nothing more is started on the card behind a fault or a hang.
LIBS=($1); R=${2:-3}; shift 2
N=${#LIBS[@]}
for r in $(seq 1 $R); do
  for k in $(seq 0 $((N - 1))); do
    L=${LIBS[$(((k + r - 1) % N))]}
    line=$(MIRHI_LIB_NAME=$L timeout -k 10 ${MIRHI_AB_LIMIT:-150} python bench.py --full --no-cpu-baseline --other-workloads c3 "$@" 2>/dev/null)
    rc=$?
    if [ $rc -ne 0 ]; then echo "$L round $r: bench.py ended with status $rc" >&2; exit $rc; fi
    echo "$line" | python -c "
import json,sys
j=json.loads(sys.stdin.readline()); rf=j['roofline']; w=j.get('workloads',{}).get('c3',{})
print('%-20s' % '$L', 'round $r', 'c2', j['value'], 'rerec4', j['rerecorded_submit']['value'], 'rerec2', j['frames_in_flight_2']['rerecorded']['value'], 'lanes2', j['frames_in_flight_2']['resubmitted']['value'],
      '| c3', w.get('value'), 'rerec4', (w.get('rerecorded_submit') or {}).get('value'), '| iso raster', rf['avg_kernel_us'], 'geometry', rf['geometry_kernel_us'], flush=True)" || exit 1
  done
done
