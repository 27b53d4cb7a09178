"""GPU (-m gpu): tools/bench_vq.py once, end to end, in a fresh child at its smallest size (3000 rows, 64 codes, 2 + 1 calls, 2
rounds): it exits 0, writes one JSON document with the keys of profiles/vq_bench.json, and every time in it is finite and
positive.  The numbers at this size are overheads and are compared with nothing.  And gaussian_point_compress.py on a 3000-row
parquet with two poses: it writes a file that loads and prints two PSNRs."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_gpu_tools_smoke import WINDOWS, structure

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("assign", "update", "iteration")


def test_bench_vq_runs_end_to_end_at_tiny_sizes(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_vq
    out = tmp_path / "result.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_vq.py"), "--rows", "3000", "--codes", "64", "--steps", "2",
                        "--warmup", "1", "--repeats", "2", "--out", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert [f.name for f in tmp_path.iterdir()] == ["result.json"]
    doc = json.loads(out.read_text())
    committed = json.load(open(os.path.join(ROOT, "profiles", "vq_bench.json")))
    assert set(doc) == set(bench_vq.KEYS) == set(committed)
    assert list(doc["sizes"]) == ["3000"] and list(doc["sizes"]["3000"]) == ["64"]
    assert sorted(committed["sizes"]) == ["2000000", "500000"] and all(sorted(v) == ["256", "4096"] for v in committed["sizes"].values())
    rec = doc["sizes"]["3000"]["64"]
    assert set(rec) == set(committed["sizes"]["500000"]["4096"])
    assert (rec["rows"], rec["codes"], rec["dim"]) == (3000, 64, 45) and rec["torch_chunk_rows"] == 3000
    for call in CALLS:
        assert set(rec[call]) == {"hip", "torch", "torch_over_hip"} and rec[call]["torch_over_hip"] > 0
        for leg in ("hip", "torch"):
            w = rec[call][leg]
            assert structure(w) == WINDOWS and w["calls_per_window"] == 2 and len(w["windows_ms"]) == 2
            for v in [w["median_ms"], w["min_ms"], w["max_ms"], *w["windows_ms"]]:
                assert math.isfinite(v) and v > 0, w
    assert rec["assign_tflops"] > 0 and 0 < rec["assign_share_of_f32_peak"] < 1
    c = doc["compress"]["3000"]
    assert set(c) == set(committed["compress"]["500000"]) and (c["rows"], c["codes"], c["iters"]) == (3000, 64, 10)
    assert all(math.isfinite(c[k]) and c[k] > 0 for k in ("compress_ms", "save_ms", "npz_bytes", "parquet_bytes", "parquet_over_npz"))
    assert c["bytes_before_deflate"] == 3000 * 35 + 64 * 90 and c["npz_bytes"] < c["parquet_bytes"]
    assert isinstance(doc["notes"], list)


def test_compress_tool_writes_a_loadable_file_and_prints_the_psnr_per_view(tmp_path):
    from taichi_3d_gaussian_splatting_amd import compression, scene_io
    from taichi_3d_gaussian_splatting_amd.synthetic import synth
    s = synth(3000, 96, 64, 0.05)
    parquet, poses, out = tmp_path / "scene.parquet", tmp_path / "poses.pt", tmp_path / "scene.npz"
    scene_io.save_parquet(str(parquet), s.point_cloud, s.point_cloud_features)
    cameras = torch.eye(4).repeat(2, 1, 1)
    cameras[1, 0, 3] = 0.2
    torch.save(cameras, str(poses))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "gaussian_point_compress.py"), str(parquet), str(out), "--codes", "64", "--iters", "3",
                        "--poses", str(poses), "--image_height", "64", "--image_width", "96", "--camera_intrinsics", "57.6", "57.6", "48", "32"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    doc = json.loads(p.stdout.strip().splitlines()[-1])
    assert len(doc["psnr"]) == 2 and all(math.isfinite(v) and v > 0 for v in doc["psnr"])
    assert doc["rows"] == 3000 and doc["codes"] == 64 and doc["bytes"] == os.path.getsize(out) < os.path.getsize(parquet) / 4
    loaded = compression.load(str(out))
    assert len(loaded) == 3000 and loaded.sh_index.dtype == np.uint8 and np.array_equal(loaded.xyz, s.point_cloud)
