#!/bin/bash
# profiles/segment_tracker.txt: timing of the segment tracker (mmsa_track_pairs alone, SegmentTracker.update() with and without tracks, a 25-class noise map
# and the one-code map against themselves as the worst cases) against mmsa_segment_pairs + mmsa_eval_panoptic, SegmentTable.update(), mmsa_eval_confusion_u8
# and the host route through numpy.unique, on two 1024 x 1024 maps and the 1080 x 1920 frame (tools/exp/segment_tracker_bench.py, which first checks every
# device result against the numpy restatement on the full-size maps).
# Needs the built library.  Each GPU step runs under its own time limit, and a step that fails ends the job.
set -eo pipefail
cd "$(dirname "$0")/../../.."
OUT="${1:-profiles/segment_tracker.txt}"
timeout -k 10 420 python tools/exp/segment_tracker_bench.py --out "$OUT" --tag "the library as built"
