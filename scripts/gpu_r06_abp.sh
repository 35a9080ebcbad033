# Round 6 A/B: sequential prefetch on uop-cache fills and the fast loop after
# coverage logging (abp/<variant>),
# bench.py --full --no-cpu (tlv headline, HEVD I/O and bare, SYN), two passes in
# opposite orders.
set -o pipefail
OUT=${OUT:-bench_out}  # where the logs go
cd "$(dirname "$0")/.." && mkdir -p $OUT/abp
for v in ${VARIANTS:-pf0 pf2 pf4 pf4 pf2 pf0}; do
  export LD_LIBRARY_PATH=$PWD/abp/$v WTFGPU_LIB=$PWD/abp/$v/libwtfgpu.so
  i=$(ls $OUT/abp | grep -c "^$v\.") 
  timeout -k 10 300 python -u bench.py --full --no-cpu > $OUT/abp/$v.$i.log 2>&1 || { echo "FAIL $v"; tail -20 $OUT/abp/$v.$i.log; exit 1; }
  tail -1 $OUT/abp/$v.$i.log > $OUT/abp/$v.$i.json
  echo "== $v"; python3 scripts/bench_brief.py $OUT/abp/$v.$i.json | grep -v "node/step\|backend/step"
done
