# Config-3 kernel timing without the CPU baseline (experiments): short-read line + long-read line.
cd $GRAFT_REPO_ROOT
O=${OUT:-bench_out}
mkdir -p $O
timeout -k 10 700 python -u bench.py --full --skip-config2 --cpu-sample 0 --steps 3 --warmup 1 "$@" > $O/qb.json 2> $O/qb.log
