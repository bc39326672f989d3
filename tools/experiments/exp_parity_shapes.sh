#!/bin/bash
# step shapes of the parity configuration, then the --full bench line: tools/experiments/exp_parity_shapes.sh <output dir, relative to the repository root>
# every bench run has its own time limit; the first one that fails ends the script
set -o pipefail
OUT=${1:?usage: tools/experiments/exp_parity_shapes.sh <output dir>}; cd "$(dirname "$0")/../.."; export TMPDIR=/tmp; mkdir -p "$OUT"
for cfg in "448 448" "896 448" "448 448"; do
  set -- $cfg
  echo "== parity (all three models): $1 videos per step, tower chunks of $2"
  timeout -k 10 600 python bench.py --precision parity --videos-per-step $1 --tower-chunk-videos $2 --steps 3 --warmup 1 --no-cpu-baseline --no-secondary --no-roofline 2> "$OUT/err_$1_$2.txt" | python -c "import sys,json; d=json.loads(sys.stdin.read()); print(d['value'], d['ms_per_step'], d['config'].get('peak_device_memory_gib'))" || { tail -3 "$OUT/err_$1_$2.txt"; exit 1; }
done 2>&1 | tee "$OUT/summary.txt" || exit 1
( time timeout -k 10 900 python bench.py --full ) > "$OUT/bench.json" 2> "$OUT/bench.err"; rc=$?; grep -E "qualified|timed region" "$OUT/bench.err"; tail -3 "$OUT/bench.err"; exit $rc
