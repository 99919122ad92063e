#!/bin/bash
# profiles/selective.txt: timing of the selective-evaluation kernel and of the thresholded map against the standalone confusion pass and the calibration
# pass (tools/exp/selective_bench.py), for the library as built and for the other same-cell merging forms and chunk size of csrc/selective.hip, each a
# build of its own (tools/build_variant.sh; it needs the objects of a regular build, so build the variants where the library was built).
# Needs the built library.  Every GPU step runs under its own time limit; a step that fails ends the job.
set -eo pipefail
cd "$(dirname "$0")/../../.."
OUT="${1:-profiles/selective.txt}"
variant() {   # <file> <flags...>: the variant library, built unless it is there already
  local so="ab/$1"; shift
  [ -f "$so" ] || tools/build_variant.sh "$so" selective.hip "$@" >&2
  echo "$PWD/$so"
}
V0=$(variant libmmsa_sel_merge0.so -DSEL_MERGE=0)
V2=$(variant libmmsa_sel_merge2.so -DSEL_MERGE=2)
VC=$(variant libmmsa_sel_chunk4096.so -DSEL_CHUNK=4096)
timeout -k 10 300 python tools/exp/selective_bench.py --out "$OUT" &&
MMSA_LIB="$V0" timeout -k 10 300 python tools/exp/selective_bench.py --append --out "$OUT" --tag "-DSEL_MERGE=0: every pixel through the two broadcast rounds" &&
MMSA_LIB="$V2" timeout -k 10 300 python tools/exp/selective_bench.py --append --out "$OUT" --tag "-DSEL_MERGE=2: four-pixel lane merge, mixed lanes through the broadcast rounds" &&
MMSA_LIB="$VC" timeout -k 10 300 python tools/exp/selective_bench.py --append --out "$OUT" --tag "-DSEL_CHUNK=4096 (SEL_MERGE as built)"
