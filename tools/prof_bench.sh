#!/usr/bin/env bash
# rocprofv3 kernel trace of the default bench command (N = 1, the --full line): bash tools/prof_bench.sh <outdir>
#   -> <outdir>/prof_bench/ (trace), <outdir>/bench_soup1m_kernel_stats.csv, <outdir>/bench_under_rocprof.json (+ .err)
set -u
here="$(cd "$(dirname "$0")/.." && pwd)"
out="$(mkdir -p "${1:?usage: tools/prof_bench.sh <outdir>}" && cd "$1" && pwd)"
export TMPDIR=/tmp
cd "$here"
timeout 900 rocprofv3 --kernel-trace --stats -d "$out/prof_bench" -o bench -- python bench.py --full --no-pmc > "$out/bench_under_rocprof.json" 2> "$out/bench_under_rocprof.err"
db=$(ls "$out"/prof_bench/*.db 2>/dev/null | head -1)
if [ -n "$db" ]; then python tools/rocpd_stats.py "$db" "$out/bench_soup1m_kernel_stats.csv" | head -6 | cut -c1-200; else echo "no rocpd database"; ls "$out/prof_bench" | head; fi
python - "$out/bench_under_rocprof.json" <<'PY'
import json
import sys
d = json.load(open(sys.argv[1]))
print("value", d["value"], "kernel_ms", d["roofline"]["kernel_ms"], d["roofline"]["kernel"])
PY
