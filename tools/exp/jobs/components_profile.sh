#!/bin/bash
# profiles/components.txt: timing of the segment passes (mmsa_components_u8 at connectivity 8 / 4 and of the label map, mmsa_component_area, suppress_small and
# the full SegmentEvaluator.add(), with a 25-class noise map as the worst case of the per-wave reduction) against mmsa_boundary_distance_u8 at cap 32 and
# mmsa_eval_confusion_u8 on the same maps, and against the host alternative (copy + scipy.ndimage.label per class), on two 1024 x 1024 maps and the
# 1080 x 1920 frame (tools/exp/components_bench.py); then, in a run of its own, a kernel trace of a short run of the same program: which of the three
# component launches holds the time.  Needs the built library.  Each GPU step runs under its own time limit.
set -eo pipefail
cd "$(dirname "$0")/../../.."
OUT="${1:-profiles/components.txt}"
TRACE="${2:-results/components_trace}"
timeout -k 10 540 python tools/exp/components_bench.py --out "$OUT"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$TRACE" -o components -- python tools/exp/components_bench.py --reps 4 --host-reps 1
