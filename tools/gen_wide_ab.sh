#!/bin/bash
# Same-box A/B of the persistent generation kernel against the per-step kernels (hipGraph replay), interleaved,
# three rounds: tools/gen_wide_ab.sh [steps]   -> the lines of profiles/r7_generation_wide.txt
cd "$(dirname "$0")/.."
STEPS=${1:-16000}
b() { python tools/gen_bench.py --steps $STEPS "$@" 2>&1 | tail -1; }
for rep in 1 2 3; do
  b --workload ref --n 1
  b --workload ref --n 1 --per-step-kernels
  b --workload ref --n 4
  b --workload ref --n 4 --per-step-kernels
  b --workload ref --batch 16
  b --workload c2 --n 1
  b --workload c2 --n 4
done
