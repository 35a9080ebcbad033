# Round 5: the driver's bench command (no CPU baselines) + a condensed view.
# $1 = tag for the output files; extra bench args via $BENCH_ARGS.
set -o pipefail
OUT=${OUT:-bench_out}  # where the logs go
R=$(cd "$(dirname "$0")/.." && pwd)
T=${1:-b}
cd $R && mkdir -p $OUT
timeout -k 10 300 python -u bench.py --full --steps 20 --warmup 5 --no-cpu $BENCH_ARGS > $OUT/r05_$T.log 2>&1 || { echo BENCH_FAIL; tail -30 $OUT/r05_$T.log; exit 1; }
python3 scripts/bench_brief.py $OUT/r05_$T.log
