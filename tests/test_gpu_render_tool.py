"""GPU (-m gpu): tools/bench_render.py once, end to end, in a fresh child with a small scene and 2 + 1 frames per leg: it exits
0 and writes one JSON document with the keys of the committed profiles/render_bench.json, every time finite and positive."""
import json
import math
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _keys(doc):
    """the document's keys, nested: {key: the same of its value}"""
    return {k: _keys(v) for k, v in doc.items()} if isinstance(doc, dict) else None


def test_bench_render_runs_end_to_end(tmp_path):
    out = tmp_path / "result.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_render.py"), "--steps", "2", "--warmup", "1", "--points", "20000",
                        "--bake-rows", "1000", "--out", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert [f.name for f in tmp_path.iterdir()] == ["result.json"]
    doc = json.loads(out.read_text())
    committed = json.load(open(os.path.join(ROOT, "profiles", "render_bench.json")))
    assert _keys(doc) == _keys(committed)
    assert list(doc["resolutions"]) == ["976x544", "1920x1088"]
    for name, legs in doc["resolutions"].items():
        w, h = (int(v) for v in name.split("x"))
        assert legs["frame_bytes_f32"] == h * w * 12 and legs["frame_bytes_u8"] == h * w * 3
        assert all(math.isfinite(v) and v > 0 for v in legs.values()), legs
    assert doc["bake"]["rows"] == 1000 and committed["bake"]["rows"] == 500_000 and committed["frames_per_leg"] >= 200
    assert all(math.isfinite(doc["bake"][k]) and doc["bake"][k] > 0 for k in ("call_ms", "torch_f32_on_device_ms", "call_gb_per_s"))
    assert 0.0 <= doc["bake"]["max_abs_difference"] < 1e-4
