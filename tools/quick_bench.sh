#!/bin/bash
# bench.py --full once, the line's essentials + the per-kernel table.  usage: bash tools/quick_bench.sh [bench args]
cd "$(dirname "$0")/.."; OUT=${OUT_DIR:-bench_out}; mkdir -p $OUT
python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline "$@" > $OUT/qb.json 2> $OUT/qb.err || tail -5 $OUT/qb.err
python - $OUT/qb.json <<'PY'
import json, sys
d = json.loads([l for l in open(sys.argv[1]) if l.startswith('{')][-1])
r = d['roofline']
print('ms/step %.3f  with input %s  gate %.1f us frac %.3f' % (d['ms_per_step'], d.get('ms_per_step_with_input'), 1e3 * r['avg_launch_ms'], r['frac']))
for k in (r.get('kernels') or []):
    print('  %-46s n/step %5.1f avg %7.1f us %6.2f ms/step %s %.3f' % (k['name'][:46], k['launches_per_step'], 1e3 * k['avg_launch_ms'], k['ms_per_step'], k['bound'], k['frac']))
PY
