# usage: bash tools/ab_libs.sh <tag> <workload> name1 name2 ...   same-box A/B of library builds build_ab/libgsrast_<name>.so (GSRAST_LIB): fps and per-kernel times, ROUNDS (default two) rounds interleaved
# bench lines go to build_ab/runs/<tag>/ with each run's stderr beside them (.log); every run has its own time limit and a run that
# fails ends the batch
set -eo pipefail
tag=$1; wl=$2; shift 2
out=build_ab/runs/$tag
mkdir -p $out
for r in $(seq 1 ${ROUNDS:-2}); do for v in "$@"; do GSRAST_LIB=$PWD/build_ab/libgsrast_$v.so timeout -k 10 300 python bench.py --full --no-cpu-baseline --breakdown-steps 50 --steps 200 --workload $wl > $out/${wl}_${v}_$r.json 2> $out/${wl}_${v}_$r.log; done; done
python - "$out" "$wl" <<'PY'
import json,glob,sys
K = ["k_filter", "k_project", "k_keygen", "k_sort_hist", "k_sort_rowscan", "k_sort_scatter", "k_blend_fwd", "k_blend_bwd_tile", "k_sum_rows"]
print("run fps", *K)
for f in sorted(glob.glob("%s/%s_*.json" % (sys.argv[1], sys.argv[2]))):
    d=json.load(open(f)); k=d.get("kernels_ms_per_view") or d["kernels_ms_per_step"]; print(f.split("/")[-1], d["value"], *[k.get(n) for n in K])
PY
