#!/bin/bash
# usage: tools/gpu_final.sh OUTDIR
# Round-end evidence run: full GPU suite, smoke, the bench with --full, and the bench command under rocprofv3 --kernel-trace --stats.
set -o pipefail
OUT=$(realpath -m "${1:?usage: tools/gpu_final.sh OUTDIR}")
mkdir -p "$OUT"
timeout -k 10 900 python -m pytest tests -m gpu -x -q > "$OUT/pytest.log" 2>&1; echo "pytest rc=$?"; tail -3 "$OUT/pytest.log"
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1; echo "smoke rc=$?"; tail -1 "$OUT/smoke.log"
timeout -k 10 600 python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err"; echo "bench rc=$?"
export TMPDIR=/tmp
R=$PWD
(cd /tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -- python3 $R/bench.py --steps 200 --warmup 20 > "$OUT/bench_prof.json" 2> "$OUT/bench_prof.err"); echo "prof rc=$?"
f=$(ls "$OUT"/prof/*/*kernel_stats.csv | head -1); head -3 $f | cut -c1-40,140-260
python - "$OUT" <<'PY'
import json, os, sys
d=json.loads(open(os.path.join(sys.argv[1], 'bench.json')).read().strip().splitlines()[-1])
print(d['value'], d['ms_per_step'], {k:v for k,v in d['roofline'].items() if k!='copy_ceiling_by_kernel_form'})
for s in d.get('secondary',[]): print(s.get('ms'), s.get('GB/s'), s.get('variant'), '|', s['workload'][:70])
print(d.get('cpu_baseline'))
PY
