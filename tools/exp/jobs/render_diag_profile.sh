#!/bin/bash
# profiles/render_diag.txt: timing of the diagnostic pictures against the mmsa_render_u8 launch on the same maps (tools/exp/render_diag_bench.py).
# Needs the built library.
set -eo pipefail
cd "$(dirname "$0")/../../.."
timeout -k 10 420 python tools/exp/render_diag_bench.py --out "${1:-profiles/render_diag.txt}"
