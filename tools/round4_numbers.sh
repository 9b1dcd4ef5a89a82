#!/bin/bash
# Round 4's numbers of record: one bench line per configuration, every line WITH its CPU legs (JSON files under gpurun_out/<tag>/).
# Usage: bash tools/round4_numbers.sh <tag> [part]     part A (default): every configuration but the large code; part B: l29k_ms_e15
# with its ~12 minutes of CPU oracle; part C: probes.
set -o pipefail
TAG=${1:-r04}
PART=${2:-A}
REPO=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$REPO/gpurun_out/$TAG
mkdir -p $OUT
cd $REPO
export PYTHONPATH=$REPO
if [ "$PART" = "A" ]; then
python bench.py --full --steps 20 --warmup 5 > $OUT/bench_h1922_ms_cs7.json 2> $OUT/bench.err && echo "bench default done" &&
python bench.py --full --steps 5 --warmup 2 --no-pipeline --cpu-sample 0 --host-steps 0 > $OUT/bench_h1922_ms_cs7_no_pipeline.json 2>> $OUT/bench.err &&
python bench.py --full --steps 5 --warmup 2 --p 0.0333 --cpu-sample 0 --host-steps 0 > $OUT/bench_h1922_ms_cs7_q0333.json 2>> $OUT/bench.err &&
python bench.py --full --steps 3 --warmup 1 --config h1922_ms_osd0 --host-steps 0 > $OUT/bench_h1922_ms_osd0.json 2>> $OUT/bench.err && echo "osd0 done" &&
python bench.py --full --steps 3 --warmup 1 --config h1922_ps_cs60 --host-steps 0 > $OUT/bench_h1922_ps_cs60_noclip.json 2>> $OUT/bench.err && echo "ps noclip done" &&
python bench.py --full --steps 3 --warmup 1 --config h1922_ps_cs60_clip20 --host-steps 0 > $OUT/bench_h1922_ps_cs60_clip20.json 2>> $OUT/bench.err && echo "ps clip20 done" &&
python bench.py --full --steps 10 --warmup 2 --config hgp400_ms_cs42 > $OUT/bench_hgp400_ms_cs42.json 2>> $OUT/bench.err && echo "hgp400 done" &&
python bench.py --full --steps 5 --warmup 2 --config hgp625_ms_cs42 --host-steps 0 > $OUT/bench_hgp625_ms_cs42.json 2>> $OUT/bench.err && echo "hgp625 done" &&
python bench.py --full --steps 5 --warmup 2 --config hgp900_ms_cs42 --host-steps 0 > $OUT/bench_hgp900_ms_cs42.json 2>> $OUT/bench.err && echo "hgp900 done"
elif [ "$PART" = "B" ]; then
python bench.py --full --steps 12 --warmup 2 --config l29k_ms_e15 --host-steps 0 > $OUT/bench_l29k_ms_e15.json 2> $OUT/bench_l29k.err && echo "l29k done"
else
python tools/bp_iteration_cost.py 1 0 > $OUT/bp_iteration_cost.txt 2>&1 &&
BP_METHOD=ps python tools/bp_iteration_cost.py 1 0 > $OUT/bp_iteration_cost_ps.txt 2>&1 &&
python tools/latency_probe.py > $OUT/latency_probe.txt 2>&1 &&
python tools/osd_probe.py 2048 > $OUT/osd_probe.txt 2>&1 &&
python tools/osd_midsize_probe.py hgp900 surface19 surface21 surface23 surface25 > $OUT/osd_midsize_probe.txt 2>&1 &&
NSL=3 python tools/host_stream_probe.py > $OUT/host_stream_probe.txt 2>&1 &&
echo "probes done"
fi
