#!/bin/bash
# profiles/boundary.txt: timing of the boundary counts (mmsa_eval_boundary_u8 at radius 1 / 3 / 8 / 32) against mmsa_eval_confusion_u8 on the same maps (the
# floor) and against the device-torch alternative (separable max_pool2d of +x and -x on both maps, then a bincount), on two 1024 x 1024 maps and the
# 1080 x 1920 frame (tools/exp/boundary_bench.py).  Needs the built library.  The one GPU step runs under its own time limit.
set -eo pipefail
cd "$(dirname "$0")/../../.."
OUT="${1:-profiles/boundary.txt}"
timeout -k 10 420 python tools/exp/boundary_bench.py --out "$OUT"
