#!/bin/bash
# profiles/rescale_class_map.txt: the one-pass rescaled class map against the canvas path (tools/exp/rescale_class_map_bench.py).  Needs the built library.
set -eo pipefail
cd "$(dirname "$0")/../../.."
timeout -k 10 300 python tools/exp/rescale_class_map_bench.py --out "${1:-profiles/rescale_class_map.txt}"
