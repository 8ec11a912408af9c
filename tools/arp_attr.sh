# Where fs_arp_flows_batch's time goes on the arp_bench.py shapes: one rocprofv3
# kernel trace with statistics, in a run of its own, over tools/arp_bench.py --shape S, summed per
# kernel (the UDP call's kernels, the ARP kernels and their sort, the runtime's fills and copies).
# usage: bash tools/arp_attr.sh [output directory] [S]     (default: bench_out/arp_attr/, c)
set -o pipefail
R="$(cd "$(dirname "$0")/.." && pwd)"
O="${1:-$R/bench_out/arp_attr}"; mkdir -p "$O"; O="$(cd "$O" && pwd)"
S="${2:-c}"
export TMPDIR=/tmp
cd /tmp
timeout -s KILL 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/trace" -o run -- \
  python3 "$R/tools/arp_bench.py" --shape "$S" --rounds 1 --launches 20 > "$O/trace.log" 2>&1 \
  || { echo "trace run failed"; tail -5 "$O/trace.log"; exit 1; }
cd "$R"
python3 - "$O" "$S" <<'PY' | tee "$O/summary.txt"
import csv, glob, re, sys
rows = []
for path in glob.glob(sys.argv[1] + "/trace/**/*kernel_stats.csv", recursive=True):
    rows += list(csv.DictReader(open(path)))
print(f"kernels of tools/arp_bench.py --shape {sys.argv[2]} --rounds 1 --launches 20 (rocprofv3 --kernel-trace --stats)")
print(f"  {'kernel':44s} {'calls':>7s} {'average us':>12s} {'min us':>10s} {'max us':>10s}")
for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
    name = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "")
    name = re.sub(r"[<(].*", "", name)
    print(f"  {name[-44:]:44s} {int(r['Calls']):7d} {float(r['AverageNs']) / 1e3:12.2f} {int(r['MinNs']) / 1e3:10.2f} "
          f"{int(r['MaxNs']) / 1e3:10.2f}")
PY
