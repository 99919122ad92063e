#!/bin/bash
# profiles/run_length.txt: timing of the run-length tables (mmsa_run_lengths_u8 / _i32 in row and column order on the class map and on the ids of its
# SegmentTable, mmsa_run_decode_i32, SegmentTable.update() with and without runs, a 25-class noise map and the one-value map as the worst cases) against
# mmsa_segment_table, mmsa_eval_confusion_u8, the transpose + row-order alternative to the column walk, and the host route through numpy, on two 1024 x 1024
# maps and the 1080 x 1920 frame (tools/exp/run_length_bench.py, which first checks every device table against the numpy restatement on the full-size map).
# Needs the built library.  Each GPU step runs under its own time limit, and a step that fails ends the job.
set -eo pipefail
cd "$(dirname "$0")/../../.."
OUT="${1:-profiles/run_length.txt}"
timeout -k 10 300 python tools/exp/run_length_bench.py --out "$OUT" --tag "the library as built"
