# rocprofv3 kernel trace + stats of the config-5 leg alone ($OUT/prof_cfg5/)
set -e
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_cfg5 -o c5 --output-format csv -- python3 bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --legs cfg5 > $OUT/prof_cfg5.log 2>&1
find $OUT/prof_cfg5 -name "*stats*"
