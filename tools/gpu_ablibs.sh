#!/bin/bash
# same-box interleaved A/B of library builds (ASR_LIB_PATH), one bench config.
# usage: tools/gpu_ablibs.sh PFX CONFIG REPS name=path ...
PFX=$1; CFG=$2; REPS=$3; shift 3
OUT=${OUT:-bench_out}   # where the logs and result lines go
mkdir -p $OUT
for i in $(seq $REPS); do
  for nv in "$@"; do
    n=${nv%%=*}; p=${nv#*=}
    ASR_LIB_PATH=$p timeout -k 10 200 python -u bench.py --full --config $CFG --steps 20 --warmup 5 --no-cpu-baseline --h2d-steps 0 > $OUT/${PFX}_${n}_$i.json 2> $OUT/${PFX}_${n}_$i.err || exit 1
    python -c "import json;d=json.load(open('$OUT/${PFX}_${n}_$i.json'));r=d['roofline'];o=r.get('other_kernels',{});print('$n', d['ms_per_step'], r.get('kernel'), r['mean_launch_us'], o.get('lstm_fwd_pass',{}).get('mean_launch_us'), o.get('gemm',{}).get('mean_launch_us'))"
  done
done
