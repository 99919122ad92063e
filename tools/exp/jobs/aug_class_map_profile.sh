#!/bin/bash
# profiles/aug_class_map.txt: the one-pass augmented class map against the canvas path (tools/exp/aug_class_map_bench.py).  Needs the built library.
set -eo pipefail
cd "$(dirname "$0")/../../.."
timeout -k 10 300 python tools/exp/aug_class_map_bench.py --out "${1:-profiles/aug_class_map.txt}"
