#!/bin/bash
# profiles/fill_nearest.txt: timing of the nearest-label fill (mmsa_fill_nearest_u8 at cap 8 / 32 / 255 on suppress_small(min_area=64, fill=254) of the class
# map, with and without the d2 output, 50 % noise holes at cap 32 and one source in an all-hole frame at cap 255 as the worst case) interleaved with
# mmsa_boundary_distance_u8 at the same caps on the same map and with mmsa_eval_confusion_u8, and the host route (copy + scipy's exact transform with indices),
# on two 1024 x 1024 maps and the 1080 x 1920 frame (tools/exp/fill_nearest_bench.py, which first checks every device result against the numpy restatement on
# the full-size map); then, in a run of its own and with no counters, a kernel trace of a short run of the fill and the distance launch at cap 32 alone: which
# of the two passes holds the time.  Needs the built library.  Each GPU step runs under its own time limit, and a step that fails ends the job.
set -eo pipefail
cd "$(dirname "$0")/../../.."
OUT="${1:-profiles/fill_nearest.txt}"
TRACE="${2:-results/fill_nearest_trace}"
timeout -k 10 420 python tools/exp/fill_nearest_bench.py --out "$OUT"
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$TRACE" -o fill_nearest -- python tools/exp/fill_nearest_bench.py --reps 4 --legs f32,d32 --no-check
python tools/exp/fill_nearest_bench.py --summarise "$TRACE" --out "$OUT"
