#!/bin/bash
# Collect HBM traffic per kernel with rocprofv3 PMC counters (separate passes, --kernel-trace only: the pool
# refuses PMC combined with other trace domains) and write profiles/pmc_traffic.json, which bench.py reads
# for roofline.traffic.  Run on the GPU box from the repo root:  bash profiles/collect_pmc.sh [workload]
# Units/corrections per /opt/skills/guides/MI355X_MICROARCH.md "HBM": FETCH_SIZE and WRITE_SIZE are in KiB;
# on gfx950 FETCH_SIZE counts 128-B fabric reads as 64 B, so reads are doubled; WRITE_SIZE is taken as is.
set -e
WL=${1:-cfg3_headline}
export TMPDIR=/tmp
OUT=gpurun_out/pmc_$WL
rm -rf $OUT
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/fetch -- python3 bench.py --full --workload $WL --steps 4 --warmup 2 --breakdown-steps 1 --no-cpu-baseline > $OUT.fetch.log 2>&1
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/write -- python3 bench.py --full --workload $WL --steps 4 --warmup 2 --breakdown-steps 1 --no-cpu-baseline > $OUT.write.log 2>&1
python3 profiles/pmc_to_json.py $WL $OUT
