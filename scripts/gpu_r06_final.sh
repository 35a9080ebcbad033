# Round 6 close: the GPU suite, smoke(), then bench.py --full (CPU
# baselines included, as the driver runs it); results under $OUT/final.
set -o pipefail
OUT=${OUT:-bench_out}  # where the logs go
cd "$(dirname "$0")/.." && mkdir -p $OUT/final
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $OUT/final/pytest_gpu.txt 2>&1 || { echo PYTEST_FAIL; tail -40 $OUT/final/pytest_gpu.txt; exit 1; }
tail -2 $OUT/final/pytest_gpu.txt
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/final/smoke.txt 2>&1 || { echo SMOKE_FAIL; tail -20 $OUT/final/smoke.txt; exit 1; }
tail -1 $OUT/final/smoke.txt
timeout -k 10 600 python -u bench.py --full > $OUT/final/bench.log 2>&1 || { echo BENCH_FAIL; tail -30 $OUT/final/bench.log; exit 1; }
tail -1 $OUT/final/bench.log > $OUT/final/bench.json
python3 scripts/bench_brief.py $OUT/final/bench.json
