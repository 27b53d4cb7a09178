"""GPU (-m gpu): tools/bench_fusion.py once, end to end, in a fresh child at tiny sizes (the 20 000-row scene at 256 x 160,
3 views, 16^3 and 24^3 voxels, 1 + 2 calls): it exits 0, writes one JSON document with the keys of profiles/fusion_bench.json,
every time in it is finite and positive, and at these sizes the torch leg runs."""
import json
import math
import os
import subprocess
import sys

import pytest

from test_gpu_tools_smoke import structure, times

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_fusion_runs_end_to_end_at_tiny_sizes(tmp_path):
    out = tmp_path / "result.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_fusion.py"), "--workload", "tiny_rehearsal", "--views", "3", "--grids", "16", "24",
                        "--steps", "2", "--warmup", "1", "--out", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert [f.name for f in tmp_path.iterdir()] == ["result.json"]
    doc = json.loads(out.read_text())
    committed = json.load(open(os.path.join(ROOT, "profiles", "fusion_bench.json")))
    assert set(doc) == set(committed)
    assert (doc["workload"], doc["views"], doc["image"], doc["n_rows"], doc["steps"]) == ("tiny_rehearsal", 3, [160, 256], 20000, 2)
    assert sorted(doc["grids"]) == ["G=16", "G=24"]
    headline = committed["grids"]["G=256"]
    for g, rec in doc["grids"].items():
        assert set(rec) == set(headline), g
        for leg in ("integrate", "isosurface"):
            assert set(structure(rec[leg])) >= set(structure(headline[leg])) - {"speedup_over_torch"}, (g, leg)
        for name in ("with_colour", "without_colour"):
            assert rec["integrate"][name]["launches"] == 1 and rec["integrate"][name]["bytes_per_second"] > 0
        assert rec["isosurface"]["vertices"] > 0 and rec["isosurface"]["faces"] > 0
        torch_leg = rec["torch_one_view_at_a_time"]
        assert torch_leg["status"] == "run", (g, torch_leg)
        assert math.isfinite(torch_leg["largest_abs_tsdf_difference_to_ours"]) and 0.0 <= torch_leg["share_of_voxels_differing"] <= 1.0
    found = list(times(doc))
    assert found, "no time in the document"
    for path, v in found:
        assert math.isfinite(v) and v > 0, (path, v)
