"""GPU (-m gpu): the tools of the bilateral grids, each once, end to end, in fresh child processes: tools/bench_bilateral.py
--quick (images of 96x64 and 52x36, two buffer sets per leg, the 20 000-row rehearsal workload, 2 + 1 calls, 2 rounds, no kernel
trace) exits 0 and writes one JSON document with the keys of profiles/bilateral_bench.json in which every window time is finite
and positive -- the numbers at this size are overheads and are compared with nothing; gaussian_point_train.py --bilateral_grid
trains a handful of iterations and writes its tables, and gaussian_point_render.py --bilateral_grid FILE corrects exactly the
frames whose image paths the file knows."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import PIL.Image
import pytest

import trainer_util as TU
from test_gpu_tools_smoke import WINDOWS, structure

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"slice": ("hip", "torch_grid_sample"), "backward": ("hip", "torch_forward_and_autograd"),
         "backward_image_only": ("hip", "torch_forward_and_autograd"), "tv": ("hip", "torch_autograd")}


def _run(script, *args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, script)] + [str(a) for a in args], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return p


def test_bench_bilateral_quick_runs_end_to_end(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_bilateral
    out = tmp_path / "result.json"
    _run(os.path.join("tools", "bench_bilateral.py"), "--quick", "--out", out)
    assert [f.name for f in tmp_path.iterdir()] == ["result.json"]
    doc = json.loads(out.read_text())
    committed = json.load(open(os.path.join(ROOT, "profiles", "bilateral_bench.json")))
    assert set(doc) == set(bench_bilateral.KEYS) == set(committed)
    assert doc["grid"] == dict(grid_x=16, grid_y=16, grid_l=8, bytes=98304) == committed["grid"]
    assert sorted(doc["calls_ms"]) == ["52x36", "96x64"]
    windows = []
    for size, rec in doc["calls_ms"].items():
        w, h = (int(v) for v in size.split("x"))
        assert set(rec) == set(CALLS) | {"height", "width", "image_mb"} and (rec["height"], rec["width"]) == (h, w)
        assert set(rec) | {"kernels_rocprofv3"} == set(next(iter(committed["calls_ms"].values())))
        for call, legs in CALLS.items():
            assert set(rec[call]) == set(legs) | {"bytes", "hbm_floor_ms", "torch_over_hip"} and rec[call]["torch_over_hip"] > 0
            windows += [rec[call][leg] for leg in legs]
        assert rec["slice"]["bytes"] == 2 * 12 * h * w and rec["backward"]["bytes"] == rec["backward_image_only"]["bytes"] == 3 * 12 * h * w
        assert rec["tv"]["bytes"] == 3 * 98304
    it = doc["training_iteration_ms"]
    assert set(it) == {"grid", "none", "grid_minus_none_ms", "grid_over_none", "workload", "height", "width"} == set(committed["training_iteration_ms"])
    assert it["workload"] == "tiny_rehearsal"
    windows += [it["grid"], it["none"]]
    for w in windows:
        assert structure(w) == WINDOWS and w["calls_per_window"] >= 1 and len(w["windows_ms"]) == 2
        for v in [w["median_ms"], w["min_ms"], w["max_ms"], *w["windows_ms"]]:
            assert math.isfinite(v) and v > 0, w
    assert isinstance(doc["notes"], list)


def test_train_script_writes_tables_the_render_script_reads(tmp_path):
    data = TU.write_dataset(tmp_path / "data", DEV, initial=TU.perturbed(TU.ground_truth_scene()))
    n_it = 4
    paths, model = data["paths"], str(tmp_path / "model")
    (tmp_path / "train.yaml").write_text(
        f"train-dataset-json-path: '{paths['train']}'\nval-dataset-json-path: '{paths['val']}'\n"
        f"pointcloud-parquet-path: '{paths['cloud']}'\nnum-iterations: {n_it}\nval-interval: {n_it - 1}\ninitial-downsample-factor: 2\n"
        f"summary-writer-log-dir: {tmp_path / 'logs'}\noutput-model-dir: {model}\nprint-metrics-to-console: False\n"
        "adaptive-controller-config:\n  num-iterations-warm-up: 1000\n")
    _run("gaussian_point_train.py", "--train_config", tmp_path / "train.yaml", "--bilateral_grid", "--bilateral_shape", 6, 4, 3, "--bilateral_tv", 5.0,
         "--bilateral_lr", 0.01)
    table_file = os.path.join(model, f"bilateral_{n_it - 1}.pt")
    assert os.path.exists(table_file) and os.path.exists(os.path.join(model, "best_bilateral.pt")) and os.path.exists(os.path.join(model, f"scene_{n_it - 1}.parquet"))
    import torch
    saved = torch.load(table_file, map_location="cpu")
    train = json.load(open(data["paths"]["train"]))
    assert tuple(saved["grids"].shape) == (len(train), 4, 6, 3, 12) and sum(saved["steps"]) == n_it and saved["image_paths"] == [r["image_path"] for r in train]
    identity = torch.tensor([1.0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
    stepped = [v for v, n in enumerate(saved["steps"]) if n]
    for v in range(len(train)):
        assert bool((saved["grids"][v] == identity).all()) == (v not in stepped)
    # the first Adam step of a view moves a value by the rate of its iteration: 0.01 at iteration 0, a hundredth of it at the end
    moved = {v: float((saved["grids"][v] - identity).abs().max()) for v in stepped}
    first = max(moved, key=moved.get)
    assert moved[first] == pytest.approx(0.01, rel=0.05) and min(moved.values()) < 0.004

    # the render script: the view of iteration 0, which the file knows, and the validation views, which it does not know
    val = json.load(open(data["paths"]["val"]))
    poses = tmp_path / "views.json"
    poses.write_text(json.dumps([train[first]] + val))
    scene = os.path.join(model, f"scene_{n_it - 1}.parquet")
    plain, corrected = tmp_path / "plain", tmp_path / "corrected"
    _run("gaussian_point_render.py", "--device", DEV, "--parquet_path", scene, "--poses", poses, "--output_prefix", plain)
    _run("gaussian_point_render.py", "--device", DEV, "--parquet_path", scene, "--poses", poses, "--output_prefix", corrected, "--bilateral_grid", table_file)
    n = 1 + len(val)
    frames = {d: [np.array(PIL.Image.open(d / f"frame_{i:03}.png")) for i in range(n)] for d in (plain, corrected)}
    for i in range(n):
        assert np.array_equal(frames[plain][i], frames[corrected][i]) == (i >= 1), i
    # a grid one Adam step of 0.01 off the identity moves an 8-bit value by a few steps at the most
    assert np.abs(frames[plain][0].astype(int) - frames[corrected][0].astype(int)).max() <= 12
    without, with_ = (json.loads((d / "metrics.json").read_text()) for d in (plain, corrected))
    assert set(without["mean"]) == {"psnr_8bit", "psnr", "ssim"} and set(with_["mean"]) == {"psnr_8bit", "psnr", "ssim", "psnr_cc"}
    assert all(np.isfinite(v["psnr_cc"]) for v in with_["views"])
    for i in range(1, n):
        assert with_["views"][i]["sse_8bit"] == without["views"][i]["sse_8bit"]
