#!/bin/bash
# profiles/panoptic.txt: timing of the panoptic passes (mmsa_segment_pairs, mmsa_eval_panoptic and the full PanopticEvaluator.add(), with 25-class noise maps
# as the worst case of the in-wave reduction and of the table) against SegmentEvaluator.add() and mmsa_eval_confusion_u8 on the same maps, on two
# 1024 x 1024 maps and the 1080 x 1920 frame (tools/exp/panoptic_bench.py); then the same program on every variant build of csrc/pairs.hip found under
# results/variants/ -- the candidates for PAIR_WAVE_ROUNDS and PAIR_MAX_PROBES, built beforehand where the objects of a regular build are, e.g.
#   tools/build_variant.sh results/variants/libmmsa_rounds8.so pairs.hip -DPAIR_WAVE_ROUNDS=8
#   tools/build_variant.sh results/variants/libmmsa_probes32.so pairs.hip -DPAIR_MAX_PROBES=32
# Needs the built library.  Each GPU step runs under its own time limit, and a step that fails ends the job.
set -eo pipefail
cd "$(dirname "$0")/../../.."
OUT="${1:-profiles/panoptic.txt}"
VARIANTS="${2:-results/variants}"
timeout -k 10 300 python tools/exp/panoptic_bench.py --out "$OUT" --tag "the library as built"
for lib in "$VARIANTS"/libmmsa_*.so; do
  [ -e "$lib" ] || continue
  tag=$(basename "$lib" .so)
  MMSA_LIB="$PWD/$lib" timeout -k 10 300 python tools/exp/panoptic_bench.py --out "${OUT%.txt}_${tag#libmmsa_}.txt" --tag "variant ${tag#libmmsa_}"
done
