"""GPU (-m gpu): tools/bench_filter3d.py once, end to end, in a fresh child at its smallest size (700 rows under 3 and 17
views, 700 and 300 rows through apply, two buffer sets per leg, the 20 000-row rehearsal workload, 2 + 1 calls, 2 rounds, no
kernel trace): it exits 0, writes one JSON document with the keys of profiles/filter3d_bench.json, and every window time in it
is finite and positive.  The numbers at this size are overheads and are compared with nothing."""
import json
import math
import os
import subprocess
import sys

import pytest

from test_gpu_tools_smoke import WINDOWS, structure

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("apply", "backward")


def test_bench_filter3d_runs_end_to_end_at_tiny_sizes(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_filter3d
    out = tmp_path / "result.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_filter3d.py"), "--rate-shapes", "700x3,700x17", "--rows", "700,300",
                        "--workload", "tiny_rehearsal", "--footprint-mb", "0", "--steps", "2", "--warmup", "1", "--repeats", "2", "--out", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert [f.name for f in tmp_path.iterdir()] == ["result.json"]
    doc = json.loads(out.read_text())
    committed = json.load(open(os.path.join(ROOT, "profiles", "filter3d_bench.json")))
    assert set(doc) == set(bench_filter3d.KEYS) == set(committed)
    windows = []
    assert sorted(doc["rate_ms"]) == ["700x17", "700x3"]
    for shape, leg in doc["rate_ms"].items():
        n, v = (int(x) for x in shape.split("x"))
        assert set(leg) == {"hip", "torch", "rows", "views", "pairs", "torch_over_hip", "hip_pairs_per_s", "device_us"}
        assert (leg["rows"], leg["views"], leg["pairs"]) == (n, v, n * v) and leg["device_us"] == "not measured" and leg["hip_pairs_per_s"] > 0
        windows += [leg["hip"], leg["torch"]]
    assert sorted(doc["apply_ms"]) == ["300", "700"]
    for rows, rec in doc["apply_ms"].items():
        assert set(rec) == {"rows", "features_mb", "apply", "backward"} and rec["rows"] == int(rows)
        for call in CALLS:
            leg = rec[call]
            assert set(leg) == {"hip", "torch", "bytes", "hbm_floor_ms", "torch_over_hip", "device_us"} and leg["torch_over_hip"] > 0
            assert leg["device_us"] == "not measured"
            windows += [leg["hip"], leg["torch"]]
        assert rec["apply"]["bytes"] == 452 * int(rows) and rec["backward"]["bytes"] == 468 * int(rows)
    it = doc["training_iteration_ms"]
    assert set(it) == {"filter", "none", "filter_minus_none_ms", "filter_over_none", "workload", "height", "width", "rows"}
    assert it["workload"] == "tiny_rehearsal" and it["rows"] == 20_000
    windows += [it["filter"], it["none"]]
    for w in windows:
        assert structure(w) == WINDOWS and w["calls_per_window"] >= 1 and len(w["windows_ms"]) == 2
        for v in [w["median_ms"], w["min_ms"], w["max_ms"], *w["windows_ms"]]:
            assert math.isfinite(v) and v > 0, w
    assert isinstance(doc["notes"], list)
