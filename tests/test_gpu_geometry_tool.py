"""GPU (-m gpu): tools/bench_geometry.py once, end to end, in a fresh child at its smallest sizes (planes of 96x64 and 52x36, two
buffer sets per size, the 20 000-row rehearsal workload, 2 + 1 calls, 2 rounds, no kernel trace, no training runs): it exits 0,
writes one JSON document with the keys of profiles/geometry_bench.json, and every window time in it is finite and positive.  The
numbers at this size are overheads and are compared with nothing.  And gaussian_point_render.py --normals_to on one pose: the PNG
it writes is geometry.depth_normals of the depth the rasteriser renders, in the 8-bit encoding."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import PIL.Image
import pytest
import torch

from test_gpu_tools_smoke import WINDOWS, structure

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEG = {"hip", "torch", "bytes", "hbm_floor_ms", "torch_over_hip"}
LEGS = {"depth_normals": 16, "normal_loss_forward": 24, "normal_loss_backward": 28, "depth_smooth_forward": 20, "depth_smooth_backward": 24}


def test_bench_geometry_runs_end_to_end_at_tiny_sizes(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_geometry
    out = tmp_path / "result.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_geometry.py"), "--sizes", "96x64,52x36", "--workload", "tiny_rehearsal",
                        "--footprint-mb", "0", "--steps", "2", "--warmup", "1", "--repeats", "2", "--out", str(out)], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert [f.name for f in tmp_path.iterdir()] == ["result.json"]
    doc = json.loads(out.read_text())
    committed = json.load(open(os.path.join(ROOT, "profiles", "geometry_bench.json")))
    assert set(doc) == set(bench_geometry.KEYS) == set(committed)
    assert doc["launches"] == committed["launches"] == {"forward": 2, "backward": 1, "depth_normals": 1}
    assert doc["tile"] == committed["tile"] == {"height": 16, "width": 64, "halo": 2}
    assert sorted(doc["kernels_ms"]) == ["52x36", "96x64"]
    windows = []
    for size, rec in doc["kernels_ms"].items():
        w, h = (int(v) for v in size.split("x"))
        assert set(rec) == {"height", "width", "plane_mb", "kernels_rocprofv3"} | set(LEGS) == set(next(iter(committed["kernels_ms"].values())))
        assert (rec["height"], rec["width"]) == (h, w) and rec["kernels_rocprofv3"] == "not measured"
        for name, bytes_per_pixel in LEGS.items():
            leg = rec[name]
            assert set(leg) == LEG and leg["torch_over_hip"] > 0 and leg["bytes"] == bytes_per_pixel * h * w
            windows += [leg["hip"], leg["torch"]]
    it = doc["training_iteration_ms"]
    assert set(it) == {"geometry", "none", "geometry_minus_none_ms", "geometry_over_none", "workload", "height", "width"} == set(committed["training_iteration_ms"])
    assert it["workload"] == "tiny_rehearsal"
    windows += [it["geometry"], it["none"]]
    for w in windows:
        assert structure(w) == WINDOWS and w["calls_per_window"] >= 1 and len(w["windows_ms"]) == 2
        for v in [w["median_ms"], w["min_ms"], w["max_ms"], *w["windows_ms"]]:
            assert math.isfinite(v) and v > 0, w
    assert isinstance(doc["notes"], list)


def test_render_tool_writes_the_normal_map_of_a_pose(tmp_path):
    from taichi_3d_gaussian_splatting_amd import geometry, scene_io
    from taichi_3d_gaussian_splatting_amd.GaussianPointRenderer import GaussianPointRenderer
    from taichi_3d_gaussian_splatting_amd.synthetic import synth, view_pose
    from taichi_3d_gaussian_splatting_amd.utils import quaternion_to_rotation_matrix_torch
    H, W = 48, 64
    scene = synth(300, W, H, 0.08, sh_deg=3, seed=0)
    parquet, poses, out = tmp_path / "scene.parquet", tmp_path / "poses.pt", tmp_path / "normals"
    scene_io.save_parquet(str(parquet), scene.point_cloud, scene.point_cloud_features)
    q, t = view_pose(1, 8)
    T = torch.eye(4)
    T[:3, :3] = quaternion_to_rotation_matrix_torch(torch.tensor(q, dtype=torch.float32))[0]
    T[:3, 3] = torch.tensor(t[0], dtype=torch.float32)
    torch.save(T[None], str(poses))
    k = [float(v) for v in (scene.camera_intrinsics[0][0], scene.camera_intrinsics[1][1], scene.camera_intrinsics[0][2], scene.camera_intrinsics[1][2])]
    args = ["--device", DEV, "--parquet_path", parquet, "--poses", poses, "--normals_to", out, "--image_height", H, "--image_width", W,
            "--camera_intrinsics", *k]
    p = subprocess.run([sys.executable, os.path.join(ROOT, "gaussian_point_render.py")] + [str(a) for a in args], cwd=tmp_path, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert json.loads(p.stdout.strip().splitlines()[-1]) == {"normals": str(out), "frames": 1}
    assert sorted(os.listdir(out)) == ["normal_000.png"]
    with PIL.Image.open(out / "normal_000.png") as im:
        assert im.mode == "RGB" and im.size == (W, H)
        stored = np.array(im)
    # the same in this process
    config = GaussianPointRenderer.GaussianPointRendererConfig(str(parquet), T[None], device=DEV)
    config.image_height, config.image_width = H, W
    config.camera_intrinsics = torch.tensor([[k[0], 0.0, k[2]], [0.0, k[1], k[3]], [0.0, 0.0, 1.0]])
    renderer = GaussianPointRenderer(config)
    q_rows, t_rows = renderer.pose_rows()
    _, depth = renderer.render(q_rows[0], t_rows[0], depth=True)
    normals = geometry.depth_normals(depth.contiguous(), tuple(k), 0.1)
    assert np.array_equal(stored, geometry.normals_to_uint8(normals).cpu().numpy())
    has = stored.any(axis=2)
    assert 0.01 < has.mean() < 1.0 and np.median(stored[has][:, 2].astype(int)) < 128          # a surface, and most of it faces along -z
