# the final tree's GPU suite, smoke() and --full bench line: tools/experiments/final_check.sh <output dir, relative to the repository root>
# every step has its own time limit; the first one that fails ends the script
OUT=${1:?usage: tools/experiments/final_check.sh <output dir>}; cd "$(dirname "$0")/../.."; export TMPDIR=/tmp; mkdir -p "$OUT"
( time timeout -k 10 1500 python -m pytest tests/ -x -q -m gpu ) > "$OUT/gpu_tests.txt" 2>&1; rc=$?; tail -5 "$OUT/gpu_tests.txt"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.txt" 2>&1; rc=$?; echo "smoke rc=$rc"; tail -3 "$OUT/smoke.txt"; [ $rc -eq 0 ] || exit $rc
( time timeout -k 10 900 python bench.py --full ) > "$OUT/bench.json" 2> "$OUT/bench.err"; rc=$?; tail -c 1500 "$OUT/bench.json"; tail -5 "$OUT/bench.err"; exit $rc
