OUT=${1:?usage: tools/exp/run_last.sh <output dir>}
mkdir -p "$OUT"
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -1
(time python bench.py --full) > "$OUT/bench_line_full.json" 2> "$OUT/bench_full_stderr.log"
tail -4 "$OUT/bench_full_stderr.log"
python - "$OUT/bench_line_full.json" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d['ms_per_step'], d['roofline'])
print([ (c['config'][:30], c.get('device_resident_ms'), c.get('create_ms')) for c in d['configs']])
PY
