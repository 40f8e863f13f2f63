#!/bin/bash
# end-of-round check on the GPU box: smoke(), the --full bench line (wall time), the whole GPU suite
#     bash tools/validate_round.sh [outdir]      (repo root; outdir defaults to build/validate)
OUT=${1:-build/validate}
mkdir -p "$OUT"
S=$(date +%s)
timeout -k 10 300 python __graft_entry__.py smoke 2>&1 | tail -1
timeout -k 10 600 python bench.py --full > "$OUT/bench_full.json" 2> "$OUT/bench_full.err"
echo "bench rc=$? wall=$(( $(date +%s) - S ))s"
python - "$OUT/bench_full.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d["value"], d["train"]["ms_per_step"], d["cpu_baseline"], d["roofline"]["frac"], (d.get("resnet50_variant") or {}).get("value"))
PY
timeout -k 10 500 python -m pytest tests -m gpu -x -q 2>&1 | tail -2
