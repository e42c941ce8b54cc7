#!/bin/bash
O=${OI_OUT_DIR:-dbg_out}
mkdir -p "$O"
{
time (timeout 600 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -3)
time (timeout 900 python bench.py --full > "$O/bench_final.json" 2> "$O/bench_final.err"; tail -c 600 "$O/bench_final.json")
OI_OUT_DIR="$O" python - <<'PY'
import json, os
d = json.loads(open(os.path.join(os.environ['OI_OUT_DIR'], 'bench_final.json')).read().strip().splitlines()[-1])
print(d['value'], d['ms_per_step'], d['roofline']['traffic'], d['roofline'].get('hbm'), d['training']['it_per_s'], d['training']['d_step']['ms'])
PY
} > "$O/smoke.log" 2>&1 < /dev/null
