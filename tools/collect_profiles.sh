# Official per-round measurement pass on an MI355X; every output goes under OUT (default out/).
#   [OUT=dir] bash tools/collect_profiles.sh r04
set -e
TAG=${1:-r04}
OUT=${OUT:-out}
export TMPDIR=/tmp && cd "$(dirname "$0")/.."
B="python3 bench.py --steps 5 --warmup 2 --full --no-cpu-baseline --no-f32"
mkdir -p "$OUT"
echo "[1/10] full bench"; python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err
echo "[2/10] sustained: one complete 1000-step run"; python bench.py --steps 1000 --warmup 5 --no-cpu-baseline --no-f32 > $OUT/bench_1000.json 2> $OUT/bench_1000.err
echo "[3/10] kernel trace"; rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -- $B > $OUT/prof_$TAG.log 2>&1
echo "[4/10] FETCH_SIZE"; rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_${TAG}_fetch -- $B > $OUT/pmc_fetch.log 2>&1
echo "[5/10] WRITE_SIZE"; rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_${TAG}_write -- $B > $OUT/pmc_write.log 2>&1
echo "[6/10] SQ pass 1"; rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_WAVE_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $OUT/pmc_${TAG}_sq1 -- $B > $OUT/pmc_sq1.log 2>&1
echo "[7/10] SQ pass 2"; rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAIT_ANY SQ_LDS_IDX_ACTIVE --output-format csv -d $OUT/pmc_${TAG}_sq2 -- $B > $OUT/pmc_sq2.log 2>&1
echo "[8/10] TCC"; rocprofv3 --kernel-trace --pmc TCC_HIT_sum TCC_MISS_sum --output-format csv -d $OUT/pmc_${TAG}_tcc -- $B > $OUT/pmc_tcc.log 2>&1
echo "[9/10] cfg3 kernel trace"; rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${TAG}_cfg3 -- $B --workload cfg3 > $OUT/prof_${TAG}_cfg3.log 2>&1
echo "[10/10] other workloads, shapes, layers"
for w in cfg3 cfg4 cfg5; do python bench.py --workload $w --steps 10 --warmup 3 --full --no-cpu-baseline --no-f32 > $OUT/bench_$w.json 2>/dev/null; done
for w in cfg2 cfg3; do
  python bench.py --workload $w --steps 8 --warmup 3 --no-cpu-baseline --no-f32 --shapes $OUT/shapes_$w.csv --layers $OUT/layers_$w.csv > /dev/null 2>&1
  python tools/shapes_table.py $OUT/shapes_$w.csv --top 80 > $OUT/${TAG}_shapes_$w.md
  python tools/layer_table.py $OUT/layers_$w.csv > $OUT/${TAG}_layers_$w.md
done
python tools/summarize_profiles.py --tag $TAG --stats $OUT/prof_$TAG --fetch $OUT/pmc_${TAG}_fetch --write $OUT/pmc_${TAG}_write --steps-in-trace 8 --out $OUT/profiles_$TAG
python tools/summarize_profiles.py --tag $TAG --stats $OUT/prof_${TAG}_cfg3 --steps-in-trace 8 --workload cfg3 --out $OUT/profiles_$TAG
python tools/summarize_pmc.py --tag $TAG --out $OUT/profiles_$TAG $OUT/pmc_${TAG}_sq1 $OUT/pmc_${TAG}_sq2 $OUT/pmc_${TAG}_tcc
find $OUT -name "*_kernel_trace.csv" -delete    # the raw traces are large: the summaries above keep what is used
find $OUT -name "*counter_collection.csv" -delete
echo done
