#!/bin/bash
# Runs on the GPU box: the GPU test suite, smoke(), the full bench line (bench.py --full).   tools/gpu_validate.sh [tag]
# Records go to $WN_RESULTS (default: results/ in the repository root).
TAG=${1:-latest}
cd "$(dirname "$0")/.."
OUT=${WN_RESULTS:-results}
mkdir -p "$OUT"
# every GPU step runs under a time limit of its own; the first step that fails, faults or times out ends the script
set -o pipefail
( time timeout -k 10 2400 python -m pytest tests -m gpu -q -x 2>&1 | tail -6 ) 2>&1 | tee "$OUT/pytest_gpu_$TAG.txt" || exit 1
timeout -k 10 180 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | grep -v amdgpu | tail -2 || exit 1
( time timeout -k 10 900 python bench.py --full 2> "$OUT/bench_$TAG.err" | tail -1 > "$OUT/bench_$TAG.json" ) 2>&1 | tail -3 || { tail -5 "$OUT/bench_$TAG.err"; exit 1; }
tail -5 "$OUT/bench_$TAG.err"
python - <<PY
import json
d = json.load(open("$OUT/bench_$TAG.json"))
e = d.get("extra", {})
print("value", d["value"], "median ms", d.get("median_ms_per_step"), "engine", d["engine_level"]["value"], "roofline", d["roofline"]["frac"], "traffic", d["roofline"]["traffic"], d["roofline"].get("traffic_kind", "")[:40], d["roofline"].get("traffic_over_algorithmic"), "verified", d["verified"])
for k, v in e.items():
    print(" ", k, {kk: v[kk] for kk in v if kk in ("samples_per_s", "hbm_frac", "kernel_variant", "verified", "ms_per_step", "mfma_peak_frac", "batched_ms", "error")})
print("cpu", d.get("cpu_baseline", {}).get("matrix"))
PY
