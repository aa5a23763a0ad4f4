#!/bin/bash
# Launch-shape sweep of the scan kernel on the GPU box: blocks, rows per iteration, nontemporal loads.
# usage: [OUT=<dir>] bash scripts/sweep_scan.sh "<blocks> <rows_per_iter> <nt>" ...   (log: $OUT/sweep.log, default bench_out/)
# --full: the roofline leg gives the scan kernel's mean duration
OUT=${OUT:-bench_out}
mkdir -p $OUT
: > $OUT/sweep.log
for cfg in "$@"; do
  set -- $cfg
  echo "=== blocks=$1 R=$2 nt=$3" >> $OUT/sweep.log
  timeout -k 10 120 python bench.py --full --steps 400 --warmup 30 --cpu-queries 0 --latency-queries 0 --scan-blocks $1 --rows-per-iter $2 --nontemporal $3 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('qps', d['value'], 'ms/step', d['ms_per_step'], 'scan_ms', d['roofline']['mean_kernel_ms'], 'frac', d['roofline']['frac'])" >> $OUT/sweep.log
done
cat $OUT/sweep.log
