# Where fs_coalesce_batch's time goes on the coalesce_bench.py shape: PMC passes of
# their own (one counter group per run, no tracing beside them) over tools/coalesce_bench.py, summed per
# dispatch of each coalesce kernel: read and write bytes against the frame and payload bytes, the
# instruction mix and the waits.
# usage: bash tools/coalesce_attr.sh [output directory]     (default: bench_out/coalesce_attr/)
set -o pipefail
R="$(cd "$(dirname "$0")/.." && pwd)"
O="${1:-$R/bench_out/coalesce_attr}"; mkdir -p "$O"; O="$(cd "$O" && pwd)"
export TMPDIR=/tmp
cd /tmp
# (FETCH_SIZE and WRITE_SIZE together ask for more TCC counters than one pass can collect)
P0="FETCH_SIZE"
P1="WRITE_SIZE TCC_EA0_WRREQ_sum TCC_EA0_WRREQ_64B_sum"
P2="SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY"
i=0
for P in "$P0" "$P1" "$P2"; do
  i=$((i+1))
  timeout -s KILL 120 rocprofv3 --pmc $P --output-format csv -d "$O/pass_$i" -o run -- \
    python3 "$R/tools/coalesce_bench.py" --rounds 1 --launches 8 > "$O/pass_$i.log" 2>&1 \
    || { echo "PMC pass $i failed"; tail -5 "$O/pass_$i.log"; exit 1; }
done
cd "$R"
python3 - "$O" <<'PY' | tee "$O/summary.txt"
import csv, glob, statistics, sys
from collections import defaultdict
per = defaultdict(float)
for path in glob.glob(sys.argv[1] + "/pass_*/**/*counter_collection.csv", recursive=True):
    for row in csv.DictReader(open(path)):
        for k in ("coalesce_classify", "coalesce_scan_partials", "coalesce_apply", "coalesce_copy"):
            if k in row["Kernel_Name"]:
                per[(k, row["Counter_Name"], path, row["Dispatch_Id"])] += float(row["Counter_Value"])
by = defaultdict(list)
for (k, name, _, _), v in per.items():
    by[(k, name)].append(v)
med = {k: statistics.median(v) for k, v in by.items()}
for (k, name) in sorted(med):
    waves = med.get((k, "SQ_WAVES"), 1) or 1
    print(f"  {k:24s} {name:24s} {med[(k, name)]:16.1f}   per wave {med[(k, name)] / waves:12.1f}")
PY
