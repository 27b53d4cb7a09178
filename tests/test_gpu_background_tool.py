"""GPU (-m gpu): tools/bench_background.py once, end to end, in a fresh child at its smallest size (images of 96x64 and 52x36,
bands 0 and 3, two buffer sets per leg, the 20 000-row rehearsal workload, 2 + 1 calls, 2 rounds, no kernel trace): it exits 0,
writes one JSON document with the keys of profiles/background_bench.json, and every window time in it is finite and positive.
The numbers at this size are overheads and are compared with nothing."""
import json
import math
import os
import subprocess
import sys

import pytest

from test_gpu_tools_smoke import WINDOWS, structure

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("composite", "backward")


def test_bench_background_runs_end_to_end_at_tiny_sizes(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_background
    out = tmp_path / "result.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_background.py"), "--sizes", "96x64,52x36", "--workload", "tiny_rehearsal",
                        "--footprint-mb", "0", "--steps", "2", "--warmup", "1", "--repeats", "2", "--out", str(out)], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert [f.name for f in tmp_path.iterdir()] == ["result.json"]
    doc = json.loads(out.read_text())
    committed = json.load(open(os.path.join(ROOT, "profiles", "background_bench.json")))
    assert set(doc) == set(bench_background.KEYS) == set(committed)
    assert sorted(doc["calls_ms"]) == ["52x36", "96x64"]
    windows = []
    for size, rec in doc["calls_ms"].items():
        w, h = (int(v) for v in size.split("x"))
        assert set(rec) == {"height", "width", "image_mb", "bands0", "bands3"} == set(next(iter(committed["calls_ms"].values())))
        assert (rec["height"], rec["width"]) == (h, w)
        for bands in ("bands0", "bands3"):
            assert set(rec[bands]) == set(CALLS)
            for call in CALLS:
                leg = rec[bands][call]
                assert set(leg) == {"hip", "torch", "bytes", "hbm_floor_ms", "torch_over_hip", "device_us"} and leg["torch_over_hip"] > 0
                assert leg["device_us"] == "not measured"
                windows += [leg["hip"], leg["torch"]]
            assert rec[bands]["composite"]["bytes"] == 28 * h * w and rec[bands]["backward"]["bytes"] == 20 * h * w
    it = doc["training_iteration_ms"]
    assert set(it) == {"sky", "none", "sky_minus_none_ms", "sky_over_none", "workload", "height", "width", "bands"} == set(committed["training_iteration_ms"])
    assert it["workload"] == "tiny_rehearsal"
    windows += [it["sky"], it["none"]]
    for w in windows:
        assert structure(w) == WINDOWS and w["calls_per_window"] >= 1 and len(w["windows_ms"]) == 2
        for v in [w["median_ms"], w["min_ms"], w["max_ms"], *w["windows_ms"]]:
            assert math.isfinite(v) and v > 0, w
    assert isinstance(doc["notes"], list)
