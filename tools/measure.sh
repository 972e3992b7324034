#!/bin/bash
# One measurement round on the GPU box: the full bench line, a rocprofv3 kernel trace of the
# same command, and FETCH_SIZE / WRITE_SIZE passes (separately, no tracing domains) of one step.
# Output under $OUT/meas/ (default bench_out/); summarise with tools/stage_profile.py and copy to profiles/.
set -e
O=${OUT:-bench_out}/meas
mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 600 python bench.py --full > $O/bench.json 2> $O/bench.err
timeout -k 10 600 rocprofv3 --kernel-trace --stats -f csv -d $O/trace -o run -- python bench.py --full \
    > $O/bench_traced.json 2> $O/bench_traced.err
timeout -k 10 300 rocprofv3 --kernel-trace --pmc FETCH_SIZE -f csv -d $O/fetch -o run -- \
    python bench.py --full --steps 1 --warmup 0 --cpu-sample 0 > $O/fetch.log 2>&1
timeout -k 10 300 rocprofv3 --kernel-trace --pmc WRITE_SIZE -f csv -d $O/write -o run -- \
    python bench.py --full --steps 1 --warmup 0 --cpu-sample 0 > $O/write.log 2>&1
