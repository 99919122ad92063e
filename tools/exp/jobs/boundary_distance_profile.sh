#!/bin/bash
# profiles/boundary_distance.txt: timing of the Euclidean boundary passes (mmsa_boundary_distance_u8 at cap 8 / 32 / 64 / 255 and the full
# EuclideanBoundaryEvaluator.add() at radius 8 / 32) against mmsa_eval_boundary_u8 at radius 8 / 32 and mmsa_eval_confusion_u8 on the same maps, and against the
# host alternative (copy + scipy's exact transform per class), on two 1024 x 1024 maps and the 1080 x 1920 frame (tools/exp/boundary_distance_bench.py).
# Needs the built library.  The one GPU step runs under its own time limit.
set -eo pipefail
cd "$(dirname "$0")/../../.."
OUT="${1:-profiles/boundary_distance.txt}"
timeout -k 10 540 python tools/exp/boundary_distance_bench.py --out "$OUT"
