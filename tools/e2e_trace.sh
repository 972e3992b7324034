# File -> TSV pipeline timeline (experiments): the e2e lines only, one trace line per batch (MTB_PIPE_TRACE).
# Usage: [E2E_ARGS=...] tools/e2e_trace.sh [tag]   (env knobs such as MTB_NO_MMAP pass through; outputs
# $OUT/e2e_trace<tag>.*, default bench_out/)
cd $GRAFT_REPO_ROOT
O=${OUT:-bench_out}
mkdir -p $O
T=${1:-}
rm -f $O/pipe_trace$T.txt
MTB_PIPE_TRACE=$O/pipe_trace$T.txt timeout -k 10 500 python -u bench.py --full --skip-config2 --cpu-sample 0 --long-reads 0 \
  --variants "" --em-pairs 0 --c5-kmers 0 --steps 1 --warmup 0 --e2e-repeat 2 $E2E_ARGS > $O/e2e_trace$T.json 2> $O/e2e_trace$T.log
