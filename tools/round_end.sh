#!/bin/bash
# Round-end measurement on the GPU box (bash tools/round_end.sh <tag> -> $MMSA_OUT_DIR/<tag>/, default results/<tag>/): full GPU suite, bench line (+cpu baseline), rocprof kernel stats, shape table, frame bench, ViT-H line, RCCL path
TAG=${1:-r02_c}
O=${MMSA_OUT_DIR:-results}/$TAG
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
mkdir -p $O
# (verbose, straight into a file under $O: a run that prints nothing for 7 minutes is taken to be hung)
timeout -k 10 1500 python -m pytest tests -x -v -m gpu --durations=10 > $O/tests_full.txt 2>&1
grep -v "^E    .*tensor(\[" $O/tests_full.txt | tail -16 > $O/tests.txt
cat $O/tests.txt
timeout 600 python bench.py --full 2> $O/bench.err | tail -1 > $O/bench.json
cat $O/bench.json | cut -c1-1200; tail -2 $O/bench.err
timeout 600 python bench.py --full --chains 1 --no-cpu-baseline 2> /dev/null | tail -1 > $O/bench_chains1.json
python -c "import json; d=json.load(open('$O/bench_chains1.json')); print('chains=1:', d['value'], d['ms_per_step'], d['encoder_only'])"
MMSA_FORCE_DIST=1 timeout 600 python bench.py --full --no-cpu-baseline --no-roofline 2> $O/dist.err | tail -1 > $O/bench_dist1.json
python -c "import json; d=json.load(open('$O/bench_dist1.json')); print('RCCL 1 rank:', d['value'], d['ms_per_step'], d['config']['collective'])" || tail -5 $O/dist.err
# (one chain: under the tracer kernels of concurrent chains no longer overlap; --no-roofline: no single-stream pass, no worst-case-precision leg -- the table is the default step only)
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -- python bench.py --steps 20 --warmup 3 --full --no-cpu-baseline --no-roofline --no-extras --chains 1 > /dev/null 2>&1
cp $(ls $O/prof/*/*kernel_stats.csv | head -1) $O/kernel_stats.csv
rm -rf $O/prof
python tools/kstats.py $O/kernel_stats.csv auto 60 > $O/kstats.txt; head -14 $O/kstats.txt
timeout 300 python tools/gemm_shapes.py > $O/shapes.txt 2>&1
head -3 $O/shapes.txt
timeout 300 python tools/frame_bench.py > $O/frame.txt 2>&1; tail -1 $O/frame.txt | cut -c1-300
timeout 400 python bench.py --config vith1024 --full --no-cpu-baseline --steps 10 --warmup 3 2> $O/vith.err | tail -1 > $O/vith.json
cat $O/vith.json | cut -c1-300
