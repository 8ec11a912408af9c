#!/bin/bash
# Kernel timing cross-check: bench.py --full, then the same under rocprofv3 --kernel-trace --stats
# (c2, c3). Output goes to $OUT/tprof (bench_out/tprof under the repository).
set -o pipefail
R="$GRAFT_REPO_ROOT"
O="$R/${OUT:-bench_out}/tprof"
mkdir -p "$O"
export TMPDIR=/tmp
cd "$R"
for cfg in c2 c3; do
  timeout -k 10 120 python bench.py --full --config $cfg --cpu-seconds 0 > "$O/plain_$cfg.json" || { echo "bench $cfg failed"; exit 1; }
  tail -1 "$O/plain_$cfg.json"
done
cd /tmp
for cfg in c2 c3; do
  timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/$cfg" -o run -- \
    python3 "$R/bench.py" --full --config $cfg --cpu-seconds 0 > "$O/bench_$cfg.json" 2> "$O/bench_$cfg.err" \
    || { echo "rocprof bench $cfg failed"; tail -5 "$O/bench_$cfg.err"; exit 1; }
done
cd "$R" && python3 tools/prof_summary.py "$O" "$O/summary"
