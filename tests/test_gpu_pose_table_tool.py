"""GPU (-m gpu): tools/bench_poses.py once, end to end, in a fresh child at its smallest sizes (5 views, the 20 000-row rehearsal
workload, 2 + 1 calls, 2 rounds, no kernel trace, no training runs): it exits 0, writes one JSON document with the keys of
profiles/pose_refine_bench.json, and every window time in it is finite and positive.  The numbers at this size are overheads
and are compared with nothing."""
import json
import math
import os
import subprocess
import sys

import pytest

from test_gpu_tools_smoke import WINDOWS, structure

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = {"hip_forward", "hip_backward", "hip_step", "torch_forward", "torch_step"}


def test_bench_poses_runs_end_to_end_at_tiny_sizes(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_poses
    out = tmp_path / "result.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_poses.py"), "--views", "5", "--workload", "tiny_rehearsal",
                        "--steps", "2", "--iteration-steps", "2", "--warmup", "1", "--repeats", "2", "--out", str(out)], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert [f.name for f in tmp_path.iterdir()] == ["result.json"]
    doc = json.loads(out.read_text())
    committed = json.load(open(os.path.join(ROOT, "profiles", "pose_refine_bench.json")))
    assert set(doc) == set(bench_poses.KEYS) == set(committed)
    assert doc["launches"] == committed["launches"] == {"compose": 1, "compose_backward": 1, "adam_step": 1}
    assert set(doc["call_ms"]) == LEGS | {"torch_step_over_hip_step", "kernels_rocprofv3"} == set(committed["call_ms"])
    assert doc["call_ms"]["kernels_rocprofv3"] == "not measured" and doc["call_ms"]["torch_step_over_hip_step"] > 0
    windows = [doc["call_ms"][name] for name in LEGS]
    assert set(doc["corrected_ms"]) == {"hip", "views"} == set(committed["corrected_ms"]) and doc["corrected_ms"]["views"] == 5
    windows.append(doc["corrected_ms"]["hip"])
    it = doc["training_iteration_ms"]
    assert set(it) == {"refined", "none", "refined_minus_none_ms", "refined_over_none", "workload", "height", "width"} == set(committed["training_iteration_ms"])
    assert it["workload"] == "tiny_rehearsal"
    windows += [it["refined"], it["none"]]
    for w in windows:
        assert structure(w) == WINDOWS and w["calls_per_window"] >= 1 and len(w["windows_ms"]) == 2
        for v in [w["median_ms"], w["min_ms"], w["max_ms"], *w["windows_ms"]]:
            assert math.isfinite(v) and v > 0, w
    assert isinstance(doc["notes"], list)
