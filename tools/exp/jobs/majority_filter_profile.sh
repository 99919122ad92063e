#!/bin/bash
# profiles/majority_filter.txt: timing of the majority filter (mmsa_majority_filter_u8 of the class map at radius 1 / 2 / 3 / 8 / 32 with and without the support
# output, the holes alone at radius 3 on suppress_small(min_area=64, fill=254) of it against mmsa_fill_nearest_u8 at cap 32, 25-value and 200-value noise as the
# worst cases) interleaved with mmsa_eval_boundary_u8 at the same radii and with mmsa_eval_confusion_u8, and the alternatives a user has (device torch: one-hot
# canvas, avg_pool2d, argmax; the host: copy + scipy), on two 1024 x 1024 maps and the 1080 x 1920 frame (tools/exp/majority_filter_bench.py, which first checks
# every device result against the numpy restatement on the full-size map); then, in a run of its own and with no counters, a kernel trace of a short run of the
# filter and the boundary pass at radius 2 and 32 alone.  Needs the built library.  Each GPU step runs under its own time limit, and a step that fails ends the job.
set -eo pipefail
cd "$(dirname "$0")/../../.."
OUT="${1:-profiles/majority_filter.txt}"
TRACE="${2:-results/majority_filter_trace}"
timeout -k 10 540 python tools/exp/majority_filter_bench.py --out "$OUT"
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$TRACE" -o majority_filter -- python tools/exp/majority_filter_bench.py --reps 4 --legs m2,b2,m32,b32 --no-check
python tools/exp/majority_filter_bench.py --summarise "$TRACE" --out "$OUT"
