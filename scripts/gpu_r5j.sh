#!/bin/bash
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
OUT=${OUT:-out}; mkdir -p "$OUT"
export PYTHONDONTWRITEBYTECODE=1
timeout 600 python bench.py --full --steps 10 --warmup 3 --profile-table --no-cpu-baseline --no-train-leg --no-shipped-leg > $OUT/ab.json 2> $OUT/ab.err
grep -v amdgpu.ids $OUT/ab.err | tail -32
python -c "
import json; r = json.loads(open('$OUT/ab.json').read().strip().splitlines()[-1]); print(round(r['value'],1), {k:(round(v['ms_per_ref_view'],3)) for k,v in r['families'].items()}, 'roofline avg_launch_ms', r['roofline']['avg_launch_ms'], 'frac', r['roofline']['frac'])"
