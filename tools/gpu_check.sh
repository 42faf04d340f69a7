#!/bin/bash
# GPU check: parity tests, then the default bench line (+ optional extra configs in $CONFIGS).
set -o pipefail
OUT=${OUT:-bench_out}   # where the logs and result lines go
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > $OUT/gpu_tests.log 2>&1 || { echo "tests failed"; tail -40 $OUT/gpu_tests.log; exit 1; }
tail -3 $OUT/gpu_tests.log
timeout -k 10 400 python -u bench.py --full > $OUT/bench.log 2>&1 || { echo "bench failed"; tail -30 $OUT/bench.log; exit 1; }
tail -1 $OUT/bench.log
for C in ${CONFIGS}; do
  timeout -k 10 400 python -u bench.py --full --config $C > $OUT/bench_$C.log 2>&1 || { echo "bench $C failed"; tail -30 $OUT/bench_$C.log; exit 1; }
  tail -1 $OUT/bench_$C.log
done
