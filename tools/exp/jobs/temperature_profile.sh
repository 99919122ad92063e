#!/bin/bash
# profiles/temperature.txt: timing of the tempered confidence kernels against their untempered siblings and of the temperature sweep against the three
# launches it stands for (tools/exp/temperature_bench.py).  Needs the built library.  The one GPU step runs under its own time limit.
set -eo pipefail
cd "$(dirname "$0")/../../.."
OUT="${1:-profiles/temperature.txt}"
timeout -k 10 420 python tools/exp/temperature_bench.py --out "$OUT"
