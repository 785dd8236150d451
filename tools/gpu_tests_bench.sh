#!/bin/bash
# GPU box: the -m gpu suite (one process) then, unless it faulted / hung / aborted, one bench run with every
# figure (--full).  Logs and the bench line go to $ECO_OUT_DIR (default bench_outputs/).
# usage: tools/gpu_tests_bench.sh [pytest selection...]
OUT="${ECO_OUT_DIR:-bench_outputs}"
mkdir -p "$OUT"
sel="${@:-tests}"
timeout -k 10 1000 python -u -m pytest $sel -m gpu -v --timeout 150 --timeout-method thread -p no:cacheprovider \
  > "$OUT/gputests.log" 2>&1
rc=$?
tail -5 "$OUT/gputests.log"
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "pytest rc=$rc: stopping"; exit $rc; fi
timeout -k 10 300 python -u bench.py --steps 10 --warmup 3 --full > "$OUT/bench.json" 2> "$OUT/bench.err"
brc=$?
cat "$OUT/bench.json"
exit $(( rc > brc ? rc : brc ))
