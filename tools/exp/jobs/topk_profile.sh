#!/bin/bash
# profiles/topk.txt: timing of the top-k launches (K = 2 / 8; the LDS form, the canvas path at a rescaled size, the recomputing form at 65 classes) against the
# confidence launch (the yardstick) and against the canvas alternative (probabilities + torch.topk), and of the evaluation pass against
# mmsa_eval_confusion_u8 (tools/exp/topk_bench.py).  Needs the built library.  The one GPU step runs under its own time limit.
set -eo pipefail
cd "$(dirname "$0")/../../.."
OUT="${1:-profiles/topk.txt}"
timeout -k 10 420 python tools/exp/topk_bench.py --out "$OUT"
