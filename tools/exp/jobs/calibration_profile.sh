#!/bin/bash
# profiles/calibration.txt: timing of the calibration kernel against the standalone confusion pass (tools/exp/calibration_bench.py).  Needs the built library.
set -eo pipefail
cd "$(dirname "$0")/../../.."
timeout -k 10 300 python tools/exp/calibration_bench.py --out "${1:-profiles/calibration.txt}"
