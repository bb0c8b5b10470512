#!/bin/bash
# The measurements of DESIGN.md 9e on the GPU box: the timing rows (K = 2 and K = 16), then ONE kernel trace for the two slot
# kernels' own times.  Every GPU step under its own time limit; a failing step ends the job.
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${1:-profiles}
mkdir -p "$OUT/track_trace"
timeout -k 10 300 python tools/bench_track.py --out "$OUT/bench_track.json" &&
timeout -k 10 300 python tools/bench_track.py --hands 16 --out "$OUT/bench_track_k16.json" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/track_trace" -o track -- \
    python tools/bench_track.py --trace --hands 16 --batches 32 &&
grep -rh --include="*kernel_stats.csv" "hand_slots" "$OUT/track_trace" | tee "$OUT/bench_track_kernels.csv"
