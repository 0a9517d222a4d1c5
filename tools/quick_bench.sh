OUT=${1:?usage: tools/quick_bench.sh <output directory>}; mkdir -p "$OUT"
python bench.py --steps 20 --warmup 5 --full --no-cpu-baseline --no-sweep > "$OUT/qb.json" 2>"$OUT/qb.err"; python - "$OUT/qb.json" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
for k in ("value","long_run","replayed_batch","index_order","hw_dispatch","queue_packed","full_lds_layout","unrelated_batches"):
    v=d.get(k); print(k, v if not isinstance(v,dict) else round(v["value"]))
PY
tail -3 "$OUT/qb.err"
