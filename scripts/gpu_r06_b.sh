# Round 6: the GPU suite, then bench.py without the CPU legs (tlv headline,
# HEVD and SYN legs) twice; one summary line per run.
set -o pipefail
OUT=${OUT:-bench_out}  # where the logs go
cd "$(dirname "$0")/.." && mkdir -p $OUT
if [ -z "$NOTESTS" ]; then
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/pytest_gpu.txt 2>&1 || { echo PYTEST_FAIL; tail -40 $OUT/pytest_gpu.txt; exit 1; }
tail -2 $OUT/pytest_gpu.txt
fi
for i in ${RUNS:-1 2}; do
  timeout -k 10 300 python -u bench.py --full --no-cpu $BENCH_ARGS > $OUT/bench_$i.log 2>&1 || { echo BENCH_FAIL; tail -30 $OUT/bench_$i.log; exit 1; }
  tail -1 $OUT/bench_$i.log > $OUT/bench_$i.json
  python3 scripts/bench_brief.py $OUT/bench_$i.json
done
