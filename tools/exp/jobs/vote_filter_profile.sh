#!/bin/bash
# profiles/vote_filter.txt: timing of the guided vote filter (mmsa_vote_filter_u8 of the class map at radius 1 / 2 / 4 / 8 / 16 with the 3-channel frame as guide,
# at radius 2 and 8 with a 1-channel guide, with weights alone, with guide and weights and on the holes of suppress_small(min_area=64, fill=254) of it, 25-value
# and 200-value noise at radius 2 and 16 as the worst cases) interleaved with mmsa_majority_filter_u8 at the same radii and with mmsa_eval_confusion_u8, and the
# device-torch composition a user had, on two 1024 x 1024 maps and the 1080 x 1920 frame (tools/exp/vote_filter_bench.py, which first checks every device
# result against the numpy restatement on the full-size map); then, in a run of its own and with no counters, a kernel trace of a short run of the filter and
# the majority filter at radius 2 and 8 alone.  With a debug-knob build of csrc/vote.hip as third argument (tools/build_variant.sh <so> vote.hip
# -DMMSA_DEBUG_KNOBS), the tile heights 8 / 16 / 32 at radius 1, 2, 4, 8 and 16 are timed with it first, each in a run of its own, and appended.
# Needs the built library.  Each GPU step runs under its own time limit, and a step that fails ends the job.
set -eo pipefail
cd "$(dirname "$0")/../../.."
OUT="${1:-profiles/vote_filter.txt}"
TRACE="${2:-results/vote_filter_trace}"
KNOBS="${3:-}"
timeout -k 10 900 python tools/exp/vote_filter_bench.py --out "$OUT"
if [ -n "$KNOBS" ]; then
  for TH in 8 16 32; do
    timeout -k 10 120 env MMSA_LIB="$KNOBS" MMSA_VOTE_TH=$TH python tools/exp/vote_filter_bench.py --reps 15 --legs g1,g2,gw2,g4,g8,gw8,g16,n200,m1,m2,m4,m8,m16 --no-check \
      --note "debug-knob build, MMSA_VOTE_TH=$TH (32 rows do not fit 64 KiB at radius 16: that leg runs with 16)" --out "$OUT.th$TH"
    { echo; echo "---- tile height $TH ----"; cat "$OUT.th$TH"; } >> "$OUT"
    rm -f "$OUT.th$TH"
  done
fi
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$TRACE" -o vote_filter -- python tools/exp/vote_filter_bench.py --reps 4 --legs g2,m2,g8,m8 --no-check
python tools/exp/vote_filter_bench.py --summarise "$TRACE" --out "$OUT"
