"""GPU (-m gpu): tools/bench_mcmc.py once, end to end, in a fresh child at its smallest size (scenes of 2000 and 3000 valid rows,
the 20 000-row rehearsal workload, 2 + 1 calls, 2 rounds): it exits 0, writes one JSON document with the keys of
profiles/mcmc_bench.json, and every window time in it is finite and positive.  The numbers at this size are overheads and are
compared with nothing."""
import json
import math
import os
import subprocess
import sys

import pytest

from test_gpu_tools_smoke import WINDOWS, structure

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"noise": ("hip", "torch"), "regulariser": ("hip", "torch_autograd"), "relocate": ("hip", "torch", "restore_only")}


def test_bench_mcmc_runs_end_to_end_at_tiny_sizes(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_mcmc
    out = tmp_path / "result.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_mcmc.py"), "--rows", "2000,3000", "--workload", "tiny_rehearsal",
                        "--steps", "2", "--warmup", "1", "--repeats", "2", "--out", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert [f.name for f in tmp_path.iterdir()] == ["result.json"]
    doc = json.loads(out.read_text())
    committed = json.load(open(os.path.join(ROOT, "profiles", "mcmc_bench.json")))
    assert set(doc) == set(bench_mcmc.KEYS) and set(committed) >= set(doc)
    assert sorted(doc["calls_ms"]) == ["2000", "3000"]
    windows = []
    for rows, rec in doc["calls_ms"].items():
        assert set(rec) == set(CALLS) | {"rows_valid", "rows_allocated", "relocate_counts"}
        assert set(rec) == set(next(iter(committed["calls_ms"].values())))
        assert rec["rows_valid"] == int(rows) and rec["rows_allocated"] == int(rows) + int(rows) // 10
        counts = rec["relocate_counts"]
        assert counts["valid_before"] == int(rows) and counts["new"] == int(rows) * 50 // 1000 and counts["dead"] > 0
        assert counts["destinations"] == counts["dead"] + counts["new"] and counts["valid_after"] == int(rows) + counts["new"]
        for call, legs in CALLS.items():
            assert set(rec[call]) == set(legs) | {"torch_over_hip"} and rec[call]["torch_over_hip"] > 0
            windows += [rec[call][leg] for leg in legs]
    it = doc["training_iteration_ms"]
    assert set(it) == {"mcmc", "adaptive", "mcmc_over_adaptive", "workload"} and it["workload"] == "tiny_rehearsal"
    windows += [it["mcmc"], it["adaptive"]]
    for w in windows:
        assert structure(w) == WINDOWS and w["calls_per_window"] >= 1 and len(w["windows_ms"]) == 2
        for v in [w["median_ms"], w["min_ms"], w["max_ms"], *w["windows_ms"]]:
            assert math.isfinite(v) and v > 0, w
    assert isinstance(doc["notes"], list)
