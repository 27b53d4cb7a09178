"""rocprofv3 --pmc output (*_counter_collection.csv) to per-kernel, per-launch averages, and the three records made of them:

    python profiles/pmc_to_json.py traffic  <workload> <dir with fetch/ and write/>   -> profiles/pmc_traffic.json (collect_pmc.sh):
        {workload: {kernel: corrected HBM bytes per launch}, workload+"_raw": {kernel: {FETCH_SIZE_KiB, WRITE_SIZE_KiB}}}
    python profiles/pmc_to_json.py sq       <workload> <dir> <dst.json>   -> SQ counters and their ratios per wave, labelled with the
        kernel sources' digest; also written to profiles/sq_counters.json, the copy bench.py reads (collect_sq.sh)
    python profiles/pmc_to_json.py counters <workload> <dir> <dst.json>   -> merged into dst.json (collect_counters.sh)
"""
import collections
import csv
import glob
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def kernel_means(csv_paths):
    """-> {kernel: {counter: mean over its launches}} of the k_* kernels in rocprofv3 counter-collection files"""
    acc = collections.defaultdict(lambda: collections.defaultdict(list))
    for path in csv_paths:
        with open(path) as fh:
            for r in csv.DictReader(fh):
                k = r["Kernel_Name"].split("(")[0].replace("void ", "").split("<")[0]
                if k.startswith("k_"):
                    acc[k][r["Counter_Name"]].append(float(r["Counter_Value"]))
    return {k: {c: sum(x) / len(x) for c, x in v.items()} for k, v in acc.items()}


def run_csvs(out_dir):
    return glob.glob(os.path.join(out_dir, "*", "*_counter_collection.csv"))


def source_digest():
    sys.path.insert(0, os.path.dirname(HERE))
    from taichi_3d_gaussian_splatting_amd import _native
    return _native.source_digest()


def dump(doc, path):
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)


def traffic(wl, out):
    means = kernel_means(run_csvs(os.path.join(out, "fetch")) + run_csvs(os.path.join(out, "write")))
    res, rawout = {}, {}
    for k, m in means.items():
        fetch, write = m.get("FETCH_SIZE", 0.0), m.get("WRITE_SIZE", 0.0)
        rawout[k] = {"FETCH_SIZE_KiB": round(fetch, 1), "WRITE_SIZE_KiB": round(write, 1)}
        res[k] = int((2.0 * fetch + write) * 1024)          # gfx950 correction: reads x2
    path = os.path.join(HERE, "pmc_traffic.json")
    data = json.load(open(path)) if os.path.exists(path) else {}
    digest = source_digest()
    if data.get("_source_digest") != digest:        # counters of another build of the kernels are dropped, not mixed in
        data = {}
    data["_source_digest"] = digest
    data[wl] = res
    data[wl + "_raw"] = rawout
    data["_note"] = ("bytes per launch = (2*FETCH_SIZE + WRITE_SIZE) * 1024; FETCH_SIZE is doubled per the gfx950 note in "
                     "MI355X_MICROARCH.md (exact for wide coalesced reads, uncalibrated for gathers); averages over the launches of "
                     "`bench.py --steps 4 --warmup 2 --breakdown-steps 1`")
    dump(data, path)
    print(json.dumps(res, indent=1))


def sq(wl, out, dst):
    res = {}
    for k, m in kernel_means(run_csvs(out)).items():
        wc = m.get("SQ_WAVE_CYCLES", 0.0) or 1.0
        res[k] = {c: round(x, 1) for c, x in m.items()}
        res[k]["valu_active_over_wave_cycles"] = round(m.get("SQ_ACTIVE_INST_VALU", 0.0) / wc, 4)
        res[k]["wait_any_over_wave_cycles"] = round(m.get("SQ_WAIT_ANY", 0.0) / wc, 4)
        res[k]["issue_stall_over_wave_cycles"] = round(m.get("SQ_WAIT_INST_ANY", 0.0) / wc, 4)
        idx = m.get("SQ_LDS_IDX_ACTIVE", 0.0)
        res[k]["lds_bank_conflict_fraction"] = round(m.get("SQ_LDS_BANK_CONFLICT", 0.0) / idx, 4) if idx else None
    doc = {"workload": wl, "source_digest": source_digest(), "note": "per-launch averages; ratios are per wave (quad-cycle units cancel)",
           "kernels": res}
    dump(doc, dst)
    dump(doc, os.path.join(os.path.dirname(os.path.abspath(dst)), "sq_counters.json"))
    for k in ("k_blend_bwd_tile", "k_blend_fwd", "k_sort_scatter", "k_bwd_points"):
        if k in res:
            print(k, {c: res[k][c] for c in res[k] if c.endswith("cycles") or c.endswith("fraction")})


def counters(wl, out, dst):
    res = {k: {c: round(x, 1) for c, x in m.items()} for k, m in kernel_means(run_csvs(out)).items()}
    old = json.load(open(dst)) if os.path.exists(dst) else {
        "workload": wl, "note": "per-launch averages over the launches of bench.py --steps 4 --warmup 2", "kernels": {}}
    for k, v in res.items():
        old["kernels"].setdefault(k, {}).update(v)
    dump(old, dst)
    for k in ("k_blend_bwd_tile", "k_blend_fwd"):
        if k in res:
            print(k, res[k])


if __name__ == "__main__":
    commands = {"traffic": traffic, "sq": sq, "counters": counters}
    if len(sys.argv) < 2 or sys.argv[1] not in commands:
        raise SystemExit(__doc__)
    commands[sys.argv[1]](*sys.argv[2:])
