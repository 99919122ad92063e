#!/bin/bash
# profiles/render.txt: timing of the render kernels against the standalone confusion pass (tools/exp/render_bench.py).  Needs the built library.
set -eo pipefail
cd "$(dirname "$0")/../../.."
timeout -k 10 300 python tools/exp/render_bench.py --out "${1:-profiles/render.txt}"
