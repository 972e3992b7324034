#!/bin/bash
# Round-3 measurement: per workload, a rocprofv3 kernel trace and separate FETCH_SIZE / WRITE_SIZE
# passes (each its own run; no tracing domains with --pmc) of one timed batch after one warm-up
# batch; summarised into profiles-ready JSON by tools/traffic_json.py.
#   gtdb     config 3: one 2M-pair batch (the bench's QuerySplit) vs the 12G-k-mer GTDB-scale DB
#   long     config 4: one 62.5k-read batch of ONT-like reads vs the same DB
#   related  config 3's "related" DB variant
#   syncmer  config 3's syncmer DB variant
#   conserved config 3's heavy-tailed "conserved" DB variant
#   config2  config 2: 1M pairs vs the 0.98G-k-mer DB
# Usage: tools/measure_r03.sh [workload ...]   (default: all). Output: gpurun_out/r03/prof/<workload>/
set -e
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
O=gpurun_out/r03/prof
mkdir -p $O
Q="--cpu-sample 0 --e2e-pairs 0 --e2e-gzip-pairs 0 --em-pairs 0 --c5-kmers 0"
declare -A CMD STEP BATCH
CMD[gtdb]="bench.py --full --skip-config2 --steps 1 --warmup 1 --long-reads 0 --variants= --gtdb-pairs 2000000 --gtdb-batch 2000000 $Q"
STEP[gtdb]=1; BATCH[gtdb]=2000000
CMD[long]="bench.py --full --skip-config2 --steps 1 --warmup 0 --gtdb-pairs 2000 --gtdb-batch 1000 --variants= --long-reads 62500 --long-batch 62500 $Q"
STEP[long]=3; BATCH[long]=62500
CMD[related]="bench.py --variant-only related --steps 1 --warmup 1 --gtdb-pairs 1000000 $Q"
STEP[related]=1; BATCH[related]=1000000
CMD[syncmer]="bench.py --variant-only syncmer --steps 1 --warmup 1 --gtdb-pairs 1000000 $Q"
STEP[syncmer]=1; BATCH[syncmer]=1000000
CMD[conserved]="bench.py --variant-only conserved --steps 1 --warmup 1 --gtdb-pairs 1000000 $Q"
STEP[conserved]=1; BATCH[conserved]=1000000
CMD[config2]="bench.py --full --gtdb-kmers 0 --steps 1 --warmup 1 --long-reads 0 $Q"
STEP[config2]=1; BATCH[config2]=1000000
W="${@:-gtdb long related syncmer conserved config2}"
for w in $W; do
  D=$O/$w
  mkdir -p $D
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -f csv -d $D/trace -o run -- python3 ${CMD[$w]} > $D/bench.json 2> $D/trace.log
  python3 tools/stage_profile.py time $D/trace/run_kernel_trace.csv ${STEP[$w]} > $D/stage_time.json
  rm -f $D/trace/run_kernel_trace.csv
  timeout -s KILL 300 rocprofv3 --kernel-trace --pmc FETCH_SIZE -f csv -d $D/fetch -o run -- python3 ${CMD[$w]} > /dev/null 2> $D/fetch.log
  python3 tools/pmc_filter.py $D/fetch
  timeout -s KILL 300 rocprofv3 --kernel-trace --pmc WRITE_SIZE -f csv -d $D/write -o run -- python3 ${CMD[$w]} > /dev/null 2> $D/write.log
  python3 tools/pmc_filter.py $D/write
  python3 tools/stage_profile.py bytes $D/fetch/run_counter_collection.csv $D/write/run_counter_collection.csv ${STEP[$w]} > $D/stage_bytes.json
  python3 tools/traffic_json.py $w $D ${BATCH[$w]} > $D/stage_traffic_$w.json
  rm -f $D/fetch/run_counter_collection.csv $D/write/run_counter_collection.csv
  echo "measured $w"
done
