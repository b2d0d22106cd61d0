#!/bin/bash
# Times the bench workload with each variant library given (names under
# bidirectional-path-tracing_amd/lib/libbdpt_amd_NAME.so; "default" = the product build).
# usage: tools/sweep_libs.sh OUT.txt NAME... [-- bench args]
cd "$(dirname "$0")/.."
OUT=$1; shift
NAMES=(); while [ $# -gt 0 ] && [ "$1" != "--" ]; do NAMES+=("$1"); shift; done
[ "$1" == "--" ] && shift
mkdir -p gpurun_out
: > $OUT
for n in "${NAMES[@]}"; do
  if [ "$n" == "default" ]; then LIB=$PWD/bidirectional-path-tracing_amd/lib/libbdpt_amd.so
  else LIB=$PWD/bidirectional-path-tracing_amd/lib/libbdpt_amd_$n.so; fi
  J=$(dirname "$OUT")/sweep_$n  # the run's JSON line and stderr, next to OUT.txt
  BDPT_AMD_LIB=$LIB timeout -k 10 150 python3 bench.py --full --no-cpu --no-parity --steps 3 --warmup 1 "$@" > $J.json 2>$J.err || { echo "$n FAILED" >> $OUT; exit 1; }
  python3 -c "import json,sys; d=json.loads(open('$J.json').read().strip().splitlines()[-1]); print('$n', d['value'], d['roofline']['kernel_ms'])" >> $OUT
  cat $OUT | tail -1
done
