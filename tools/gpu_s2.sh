#!/bin/bash
# usage: tools/gpu_s2.sh OUTDIR
set -o pipefail
OUT=$(realpath -m "${1:?usage: tools/gpu_s2.sh OUTDIR}")
mkdir -p "$OUT"
timeout -k 10 900 python -m pytest tests -m gpu -x -q > "$OUT/pytest.log" 2>&1; echo "pytest rc=$?"
tail -15 "$OUT/pytest.log"
timeout -k 10 400 python bench.py --full --no-cpu-baseline > "$OUT/bench.json" 2> "$OUT/bench.err"; echo "bench rc=$?"
python - "$OUT" <<'PY'
import json, os, sys
d=json.loads(open(os.path.join(sys.argv[1], 'bench.json')).read().strip().splitlines()[-1])
print(d['value'], d['ms_per_step'], d['roofline'])
for s in d.get('secondary',[]): print(s)
PY
