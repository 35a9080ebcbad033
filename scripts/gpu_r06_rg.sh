# Round 6: regroup launch length on the GPU-bound node (host plumbing async):
# bench.py --full --no-cpu (tlv headline + hevd / hevd_bare / syn legs) per
# --regroup-steps value given (-1 = the engine default, 1024).
set -o pipefail
OUT=${OUT:-bench_out}  # where the logs go
cd "$(dirname "$0")/.." && mkdir -p $OUT/rg
for rg in "$@"; do
  timeout -k 10 300 python -u bench.py --full --no-cpu --regroup-steps $rg $BENCH_ARGS > $OUT/rg/b_$rg.log 2>&1 || { echo BENCH_FAIL $rg; tail -20 $OUT/rg/b_$rg.log; exit 1; }
  tail -1 $OUT/rg/b_$rg.log > $OUT/rg/b_$rg.json
  echo "== regroup $rg"; python3 scripts/bench_brief.py $OUT/rg/b_$rg.json
done
