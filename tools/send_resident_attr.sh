# Where fs_send_rings_resident's time goes: one rocprofv3 kernel trace with statistics, in a
# run of its own, over tools/send_resident_bench.py's shapes (a) and (b), summed per kernel: the three plan
# kernels and the frame kernel of the resident call beside the host-socket call's one kernel.
# usage: bash tools/send_resident_attr.sh [output directory]     (default: bench_out/send_resident_attr/)
set -o pipefail
R="$(cd "$(dirname "$0")/.." && pwd)"
O="${1:-$R/bench_out/send_resident_attr}"; mkdir -p "$O"; O="$(cd "$O" && pwd)"
export TMPDIR=/tmp
cd /tmp
timeout -s KILL 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/trace" -o run -- \
  python3 "$R/tools/send_resident_bench.py" --shapes ab --rounds 1 --launches 30 > "$O/trace.log" 2>&1 \
  || { echo "trace run failed"; tail -5 "$O/trace.log"; exit 1; }
cd "$R"
python3 - "$O" <<'PY' | tee "$O/summary.txt"
import csv, glob, re, sys
rows = []
for path in glob.glob(sys.argv[1] + "/trace/**/*kernel_stats.csv", recursive=True):
    rows += list(csv.DictReader(open(path)))
print("kernels of tools/send_resident_bench.py --shapes ab --rounds 1 --launches 30 (rocprofv3 --kernel-trace --stats);")
print("the three shapes share the kernels, so min is the small-frame-count shapes' and max the 65,536 x 1,500 B ones'")
print(f"  {'kernel':44s} {'calls':>7s} {'average us':>12s} {'min us':>10s} {'max us':>10s}")
for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
    name = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "")
    name = re.sub(r"[<(].*", "", name)
    print(f"  {name[-44:]:44s} {int(r['Calls']):7d} {float(r['AverageNs']) / 1e3:12.2f} {int(r['MinNs']) / 1e3:10.2f} "
          f"{int(r['MaxNs']) / 1e3:10.2f}")
PY
