#!/bin/bash
# Arbitrary SQ/TCP/... counters for every k_* kernel of the bench, one rocprofv3 --pmc pass per call (counters in their
# own run, --kernel-trace only) under a time limit.  Run on the GPU box from the repo root:
#   bash profiles/collect_counters.sh <out.json> "<COUNTER> <COUNTER> ..." [workload]
set -eo pipefail
DST=$1
CTRS=$2
WL=${3:-cfg3_headline}
export TMPDIR=/tmp
OUT=gpurun_out/ctr_$$
rm -rf $OUT
timeout -k 10 900 rocprofv3 --kernel-trace --pmc $CTRS --output-format csv -d $OUT -- python3 bench.py --full --workload $WL --steps 4 --warmup 2 --breakdown-steps 1 --no-cpu-baseline > $OUT.log 2>&1
python3 profiles/pmc_to_json.py counters $WL $OUT $DST
rm -rf $OUT $OUT.log
