# Time k_run build variants (wtf_amd/csrc/variants/*) on the SYN bench, one process each.
set -o pipefail
OUT=${OUT:-bench_out}  # where the logs go
cd "$(dirname "$0")/.." && mkdir -p $OUT
for V in v11 v10 v21 v20; do
  WTFGPU_LIB=$PWD/wtf_amd/csrc/variants/$V/libwtfgpu.so timeout -k 10 200 python3 bench.py --full --steps 2 --warmup 1 --no-cpu $BENCH_ARGS > $OUT/var_$V.log 2>&1 || { tail -5 $OUT/var_$V.log; exit 1; }
  echo "$V"; tail -1 $OUT/var_$V.log | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print({k:d[k] for k in ('value','gpu_kernel_ms_per_step')})"
done
