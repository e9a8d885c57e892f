# The standing checks on a GPU machine: GPU test suite, smoke, the plain bench line and the --full one.
#   bash tools/gpu_round.sh [tag] [log directory, default logs]
# Each step has its own time limit and the next one starts only if it passed (a fault ends the sequence).
TAG=${1:-run}; LOG=${2:-logs}; mkdir -p "$LOG"; rm -f "$LOG"/*_"$TAG".log
timeout -k 10 1500 python -m pytest tests -m gpu -q > "$LOG/pytest_$TAG.log" 2>&1 &&
  timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$LOG/smoke_$TAG.log" 2>&1 &&
  timeout -k 10 300 python bench.py > "$LOG/bench_$TAG.log" 2>&1 &&
  timeout -k 10 900 python bench.py --full > "$LOG/bench_full_$TAG.log" 2>&1
rc=$?
for f in pytest smoke bench bench_full; do [ -f "$LOG/${f}_$TAG.log" ] && tail -6 "$LOG/${f}_$TAG.log"; done
exit $rc
