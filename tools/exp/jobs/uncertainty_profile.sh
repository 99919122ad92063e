#!/bin/bash
# profiles/uncertainty.txt: timing of the margin / entropy score launches against the confidence launch (the yardstick) and against the canvas alternative
# (probabilities + mmsa_argmax_score_nchw), and of the recomputing form at 65 classes (tools/exp/uncertainty_bench.py).  Needs the built library.  The one GPU
# step runs under its own time limit.
set -eo pipefail
cd "$(dirname "$0")/../../.."
OUT="${1:-profiles/uncertainty.txt}"
timeout -k 10 420 python tools/exp/uncertainty_bench.py --out "$OUT"
