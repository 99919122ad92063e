#!/bin/bash
# profiles/segment_table.txt: timing of the segment table (mmsa_segment_table with and without values, its prefix-sum launches apart from its accumulate
# launch, the full SegmentTable.update(), mmsa_select_segments_u8, the one-code map and a 25-class noise map as the worst cases) against mmsa_component_area,
# suppress_small, SegmentEvaluator.add() and the host route through scipy, on two 1024 x 1024 maps and the 1080 x 1920 frame
# (tools/exp/segment_table_bench.py, which first checks the device table against scipy.ndimage on the full-size map); then the same program on every variant
# build of csrc/segtable.hip found under results/variants/ -- the candidates for SEGTAB_WAVE_ROUNDS and SEGTAB_BLOCK, built beforehand where the objects of a
# regular build are, e.g.
#   tools/build_variant.sh results/variants/libmmsa_rounds2.so segtable.hip -DSEGTAB_WAVE_ROUNDS=2
#   tools/build_variant.sh results/variants/libmmsa_block4096.so segtable.hip -DSEGTAB_BLOCK=4096
# (a variant named block<N> is run with --block N: the Python layer sizes the scratch of the prefix sum by it).
# Needs the built library.  Each GPU step runs under its own time limit, and a step that fails ends the job.
set -eo pipefail
cd "$(dirname "$0")/../../.."
OUT="${1:-profiles/segment_table.txt}"
VARIANTS="${2:-results/variants}"
timeout -k 10 300 python tools/exp/segment_table_bench.py --out "$OUT" --tag "the library as built"
for lib in "$VARIANTS"/libmmsa_*.so; do
  [ -e "$lib" ] || continue
  tag=$(basename "$lib" .so)
  tag=${tag#libmmsa_}
  block=()
  case "$tag" in block*) block=(--block "${tag#block}") ;; esac
  MMSA_LIB="$PWD/$lib" timeout -k 10 300 python tools/exp/segment_table_bench.py --no-host "${block[@]}" --out "${OUT%.txt}_${tag}.txt" --tag "variant $tag"
done
