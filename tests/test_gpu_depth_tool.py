"""GPU (-m gpu): tools/bench_depth_loss.py once, end to end, in a fresh child at its smallest sizes (planes of 96x64 and 52x36,
two buffer sets per leg, the 20 000-row rehearsal workload, 2 + 1 calls, 2 rounds, no kernel trace, no training runs): it exits
0, writes one JSON document with the keys of profiles/depth_loss_bench.json, and every window time in it is finite and
positive.  The numbers at this size are overheads and are compared with nothing."""
import json
import math
import os
import subprocess
import sys

import pytest

from test_gpu_tools_smoke import WINDOWS, structure

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEG = {"hip", "torch", "bytes", "hbm_floor_ms", "torch_over_hip"}


def test_bench_depth_loss_runs_end_to_end_at_tiny_sizes(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_depth_loss
    out = tmp_path / "result.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_depth_loss.py"), "--sizes", "96x64,52x36", "--workload", "tiny_rehearsal",
                        "--footprint-mb", "0", "--steps", "2", "--warmup", "1", "--repeats", "2", "--out", str(out)], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert [f.name for f in tmp_path.iterdir()] == ["result.json"]
    doc = json.loads(out.read_text())
    committed = json.load(open(os.path.join(ROOT, "profiles", "depth_loss_bench.json")))
    assert set(doc) == set(bench_depth_loss.KEYS) == set(committed)
    assert doc["launches"] == committed["launches"] == {"forward": 2, "forward_align": 4, "backward": 1, "resample": 1}
    assert sorted(doc["loss_ms"]) == ["52x36", "96x64"]
    windows = []
    for size, rec in doc["loss_ms"].items():
        w, h = (int(v) for v in size.split("x"))
        assert set(rec) - {"kernels_rocprofv3"} == {"height", "width", "plane_mb", "metric", "relative"} and (rec["height"], rec["width"]) == (h, w)
        assert set(rec) | {"kernels_rocprofv3"} == set(next(iter(committed["loss_ms"].values())))
        for mode, passes in (("metric", 1), ("relative", 2)):
            assert set(rec[mode]) == {"forward", "backward"}
            for call, leg in rec[mode].items():
                assert set(leg) == LEG and leg["torch_over_hip"] > 0
                windows += [leg["hip"], leg["torch"]]
            assert rec[mode]["forward"]["bytes"] == passes * 12 * h * w and rec[mode]["backward"]["bytes"] == 16 * h * w
    assert doc["loss_ms"]["96x64"]["kernels_rocprofv3"] == "not measured"
    assert sorted(doc["resample_ms"]) == ["factor_1", "factor_2", "factor_4"] == sorted(committed["resample_ms"])
    for name, leg in doc["resample_ms"].items():
        assert set(leg) == LEG | {"source", "height", "width"} == set(committed["resample_ms"][name])
        assert leg["bytes"] == 96 * 64 * 2 + 8 * leg["height"] * leg["width"]
        windows += [leg["hip"], leg["torch"]]
    assert (doc["resample_ms"]["factor_2"]["height"], doc["resample_ms"]["factor_2"]["width"]) == (32, 48)
    it = doc["training_iteration_ms"]
    assert set(it) == {"metric", "none", "metric_minus_none_ms", "metric_over_none", "workload", "height", "width"} == set(committed["training_iteration_ms"])
    assert it["workload"] == "tiny_rehearsal"
    windows += [it["metric"], it["none"]]
    for w in windows:
        assert structure(w) == WINDOWS and w["calls_per_window"] >= 1 and len(w["windows_ms"]) == 2
        for v in [w["median_ms"], w["min_ms"], w["max_ms"], *w["windows_ms"]]:
            assert math.isfinite(v) and v > 0, w
    assert isinstance(doc["notes"], list)
