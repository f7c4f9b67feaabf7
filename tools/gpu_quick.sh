#!/bin/bash
# quick GPU visit: kernel + model parity tests, the --full bench line, single-stream kernel stats; output in $OUT_DIR (default bench_out/)
cd "$(dirname "$0")/.."; export OUT_DIR=${OUT_DIR:-bench_out}; mkdir -p $OUT_DIR
timeout 1200 python -m pytest tests/test_gpu_kernels.py tests/test_gpu_model.py tests/test_gpu_fullsize.py tests/test_gpu_configs.py -m gpu -q -x --no-header -p no:cacheprovider 2>&1 | tail -6
timeout 300 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $OUT_DIR/bench_q.json 2> $OUT_DIR/bench_q.err; python - $OUT_DIR/bench_q.json <<'PY'
import json, sys
d = json.loads([l for l in open(sys.argv[1]) if l.startswith('{')][-1]); r = d['roofline']
print('bench: ms/step %.3f  %.4g samples/s | gate kernel %.1f TF frac %.3f avg %.1f us' % (d['ms_per_step'], d['value'], r['achieved'], r['frac'], 1e3 * r['avg_launch_ms']))
PY
bash tools/kstats.sh --no-overlap 2>&1 | head -16
