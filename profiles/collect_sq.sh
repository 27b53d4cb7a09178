#!/bin/bash
# SQ counters of every kernel of the bench (one rocprofv3 PMC pass, --kernel-trace only, under a time limit), summarised per
# kernel into profiles/<tag>_sq_counters.json.  Run on the GPU box from the repo root:  bash profiles/collect_sq.sh r01_e [workload]
# SQ_WAVE_CYCLES / SQ_ACTIVE_INST_* / SQ_WAIT_* count quad-cycles per wave (MI355X_MICROARCH.md, "rocprofv3 PMC slots").
set -eo pipefail
TAG=${1:-r01}
WL=${2:-cfg3_headline}
export TMPDIR=/tmp
OUT=gpurun_out/sq_$WL
rm -rf $OUT
timeout -k 10 900 rocprofv3 --kernel-trace --pmc SQ_WAVE_CYCLES SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_ANY SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_INSTS_VALU SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE \
    --output-format csv -d $OUT -- python3 bench.py --full --workload $WL --steps 4 --warmup 2 --breakdown-steps 1 --no-cpu-baseline > $OUT.log 2>&1
python3 profiles/pmc_to_json.py sq $WL $OUT profiles/${TAG}_sq_counters.json
rm -rf $OUT
