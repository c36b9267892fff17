d=${OUT_DIR:-/tmp/r6_final}/${OUT:-r6x}
mkdir -p "$d"
timeout 2400 python -m pytest tests -x -q -m gpu > "$d/gpu_tests.log" 2>&1
tail -3 "$d/gpu_tests.log"
for i in 1 2 3; do
timeout 1200 python bench.py --full > "$d/bench$i.json" 2> "$d/bench$i.err"
python scripts/bench_fields.py "$d/bench$i.json"
done
