"""Cost of the pose gradient (k_pose.hip) at cfg3_headline: forward + backward of sum(g * image) in three modes --
points only, points + pose, pose only -- at n_objects = 1 and 8 (points split into 8 objects with equal poses).
Device events time the steps; `--rocprof` adds one `rocprofv3 --kernel-trace --stats` run of a child process for the
per-kernel times.  Writes profiles/pose_grad_bench.json (or --out).

    python tools/bench_pose_grad.py [--steps 50] [--warmup 10] [--rocprof] [--out PATH]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from taichi_3d_gaussian_splatting_amd import CameraInfo, GaussianPointCloudRasterisation as Rast   # noqa: E402
from taichi_3d_gaussian_splatting_amd.synthetic import CONFIGS, synth, view_pose                    # noqa: E402

MODES = {"points": (True, False), "points+pose": (True, True), "pose": (False, True)}


def make(n_objects, dev):
    s = synth(**CONFIGS["cfg3_headline"])
    q, t = view_pose()
    if n_objects > 1:
        s.point_object_id[:] = np.random.default_rng(1).integers(0, n_objects, s.point_object_id.shape[0]).astype(np.int32)
    q, t = np.repeat(q, n_objects, 0), np.repeat(t, n_objects, 0)
    return s, q, t


def step_fn(s, q, t, mode, dev):
    points, pose = MODES[mode]
    module = Rast(Rast.GaussianPointCloudRasterisationConfig())
    pc = torch.tensor(s.point_cloud, device=dev, requires_grad=points)
    feat = torch.tensor(s.point_cloud_features, device=dev, requires_grad=points)
    qq = torch.tensor(q, device=dev, requires_grad=pose)
    tt = torch.tensor(t, device=dev, requires_grad=pose)
    inp = Rast.GaussianPointCloudRasterisationInput(
        point_cloud=pc, point_cloud_features=feat, point_object_id=torch.tensor(s.point_object_id, device=dev),
        point_invalid_mask=torch.tensor(s.point_invalid_mask, device=dev),
        camera_info=CameraInfo(camera_intrinsics=torch.tensor(s.camera_intrinsics, device=dev), camera_height=s.height,
                               camera_width=s.width, camera_id=0),
        q_pointcloud_camera=qq, t_pointcloud_camera=tt, color_max_sh_band=3)
    g = torch.full((s.height, s.width, 3), 1e-3, device=dev)

    def step():
        for x in (pc, feat, qq, tt):
            x.grad = None
        image = module(inp)[0]
        image.backward(g)
    return step


def time_mode(s, q, t, mode, steps, warmup, dev):
    step = step_fn(s, q, t, mode, dev)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        step()
        b.record()
    torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in ev])
    return dict(ms_median=float(np.median(ms)), ms_p10=float(np.percentile(ms, 10)), ms_p90=float(np.percentile(ms, 90)), steps=steps)


def child(steps):
    """rocprofv3 target: every mode at both object counts, `steps` steps each."""
    dev = torch.device("cuda:0")
    for n_objects in (1, 8):
        s, q, t = make(n_objects, dev)
        for mode in MODES:
            step = step_fn(s, q, t, mode, dev)
            for _ in range(steps):
                step()
    torch.cuda.synchronize()


def rocprof(steps):
    out = tempfile.mkdtemp(prefix="pose_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "run", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--child", str(steps)]
    subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
    stats = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    rows = {}
    if stats:
        for r in csv.DictReader(open(stats[0])):
            name = r.get("Name", "")
            if any(k in name for k in ("k_pose", "k_bwd_points", "k_sum_rows", "k_blend_bwd_tile")):
                rows[name.split("(")[0]] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_grad_bench.json"))
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child)
        return
    dev = torch.device("cuda:0")
    res = {"workload": "cfg3_headline", "step": "forward + backward of sum(g * image)", "device": torch.cuda.get_device_name(0),
           "modes": {}}
    for n_objects in (1, 8):
        s, q, t = make(n_objects, dev)
        for mode in MODES:
            res["modes"][f"{mode}@kobj{n_objects}"] = time_mode(s, q, t, mode, a.steps, a.warmup, dev)
    if a.rocprof:
        res["kernels_rocprofv3"] = rocprof(10)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
