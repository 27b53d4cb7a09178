#!/bin/bash
# Collect HBM traffic per kernel with rocprofv3 PMC counters (separate passes, --kernel-trace only: counters are never
# combined with another trace domain; each pass under a time limit) and write profiles/pmc_traffic.json, which bench.py
# reads for roofline.traffic.  Run on the GPU box from the repo root:  bash profiles/collect_pmc.sh [workload]
# Units/corrections: FETCH_SIZE and WRITE_SIZE are in KiB; on gfx950 FETCH_SIZE counts 128-B fabric reads as 64 B, so
# reads are doubled; WRITE_SIZE is taken as is.
set -eo pipefail
WL=${1:-cfg3_headline}
export TMPDIR=/tmp
OUT=gpurun_out/pmc_$WL
rm -rf $OUT
timeout -k 10 900 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/fetch -- python3 bench.py --full --workload $WL --steps 4 --warmup 2 --breakdown-steps 1 --no-cpu-baseline > $OUT.fetch.log 2>&1
timeout -k 10 900 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/write -- python3 bench.py --full --workload $WL --steps 4 --warmup 2 --breakdown-steps 1 --no-cpu-baseline > $OUT.write.log 2>&1
python3 profiles/pmc_to_json.py traffic $WL $OUT
