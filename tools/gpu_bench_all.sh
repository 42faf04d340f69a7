#!/bin/bash
# Every bench config once (default steps), for DESIGN.md numbers
set -o pipefail
OUT=${OUT:-bench_out}   # where the logs and result lines go
mkdir -p $OUT
for C in ${CONFIGS:-ctc5x512 timit2x320 att4x320 hybrid4x320 vgg_hier}; do
  timeout -k 10 400 python -u bench.py --full --config $C ${EXTRA} > $OUT/bench_$C.log 2>&1 || { echo "bench $C failed"; tail -20 $OUT/bench_$C.log; exit 1; }
  tail -1 $OUT/bench_$C.log | cut -c1-330
done
