OUT=${1:?usage: tools/exp/run_full.sh <output dir>}
mkdir -p "$OUT"
timeout 1500 python -m pytest tests -x -q -m gpu > "$OUT/pytest_gpu.log" 2>&1
tail -4 "$OUT/pytest_gpu.log"
timeout 900 python bench.py --full > "$OUT/bench_line.json" 2> "$OUT/bench_stderr.log"
python - "$OUT/bench_line.json" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d['ms_per_step'], d['roofline']['frac'], d['roofline'].get('traffic'))
for c in d['configs']:
    for k in c:
        if 'create_ms' in str(c[k]) or k=='create_ms': print(k, str(c[k])[:400])
print(json.dumps(d['batch'].get('one_old_many_new'))[:500])
PY
grep -o '"create_ms[^}]*}' "$OUT/bench_line.json" | head -3
