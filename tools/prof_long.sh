cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
O=${OUT:-bench_out}; mkdir -p $O
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $O/prof_long -o run -- python3 bench.py --full --skip-config2 --gtdb-pairs 2000 --gtdb-batch 1000 --steps 1 --warmup 1 --cpu-sample 0 --long-reads 50000 > $O/prof_long.json 2> $O/prof_long.log
