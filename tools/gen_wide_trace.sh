#!/bin/bash
# rocprofv3 kernel trace (no counters) of the reference-default decoder on the persistent road: one warm-up launch of
# 64 steps and one 4096-step chunk -> expect two gen_mega_kernel dispatches and two one-off pack launches
cd "$(dirname "$0")/.."
OUT=${1:-/tmp/gen_wide_trace}
rm -rf "$OUT"
timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT" -o gen -- python tools/gen_bench.py --workload ref --steps 4096 2>&1 | grep workload
s=$(find "$OUT" -name "*kernel_stats.csv" | head -1)
[ -n "$s" ] || { echo "no stats file"; exit 1; }
python - "$s" <<'PY'
import csv, sys
for r in csv.DictReader(open(sys.argv[1])):
    if 'gen_' in r['Name']:
        print('%-70s calls %5s  total %12.1f us  avg %12.1f us' % (r['Name'][:70], r['Calls'], float(r['TotalDurationNs']) / 1e3, float(r['AverageNs']) / 1e3))
PY
