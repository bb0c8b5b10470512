#!/bin/bash
# The measurements of DESIGN.md 9f on the GPU box: the timing rows (N x K = 1 x 2, 32 x 2, 32 x 16), then ONE kernel trace for the
# two mesh kernels' own times.  Every GPU step under its own time limit; a failing step ends the job.
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${1:-profiles}
mkdir -p "$OUT/smooth_trace"
timeout -k 10 400 python tools/bench_smooth.py --out "$OUT/bench_smooth.json" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/smooth_trace" -o smooth -- \
    python tools/bench_smooth.py --trace --shapes 32x16 &&
grep -rh --include="*kernel_stats.csv" "mesh_finish" "$OUT/smooth_trace" | tee "$OUT/bench_smooth_kernels.csv"
