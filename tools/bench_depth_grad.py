"""Cost of the differentiable depth / accumulated alpha (gs_backward_ex) at cfg3_headline: forward + backward in three modes --
image only (gs_backward, today's path), image + depth (config.differentiable_depth) and image + depth + alpha
(forward(..., return_accumulated_alpha=True)).  Device events time the steps; `--rocprof` adds one
`rocprofv3 --kernel-trace --stats` run of a child process per mode for the per-kernel times (the AUX instantiations show up
under their template arguments).  Writes profiles/depth_grad_bench.json (or --out).

    python tools/bench_depth_grad.py [--steps 50] [--warmup 10] [--rocprof] [--out PATH]
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

MODES = ["image", "image+depth", "image+depth+alpha"]


def make():
    s = synth(**CONFIGS["cfg3_headline"])
    q, t = view_pose()
    return s, q, t


def step_fn(s, q, t, mode, dev):
    cfg = Rast.GaussianPointCloudRasterisationConfig()
    cfg.differentiable_depth = mode != "image"
    module = Rast(cfg)
    alpha = mode.endswith("alpha")
    pc = torch.tensor(s.point_cloud, device=dev, requires_grad=True)
    feat = torch.tensor(s.point_cloud_features, device=dev, requires_grad=True)
    inp = Rast.GaussianPointCloudRasterisationInput(
        point_cloud=pc, point_cloud_features=feat, point_object_id=torch.tensor(s.point_object_id, device=dev),
        point_invalid_mask=torch.tensor(s.point_invalid_mask, device=dev),
        camera_info=CameraInfo(camera_intrinsics=torch.tensor(s.camera_intrinsics, device=dev), camera_height=s.height,
                               camera_width=s.width, camera_id=0),
        q_pointcloud_camera=torch.tensor(q, device=dev), t_pointcloud_camera=torch.tensor(t, device=dev), color_max_sh_band=3)
    g = torch.full((s.height, s.width, 3), 1e-3, device=dev)
    gd = torch.full((s.height, s.width), 1e-3, device=dev)
    ga = torch.full((s.height, s.width), -1e-3, device=dev)

    def step():
        pc.grad = feat.grad = None
        outs = module(inp, return_accumulated_alpha=alpha)
        if mode == "image":
            outs[0].backward(g)
        elif mode == "image+depth":
            torch.autograd.backward([outs[0], outs[1]], [g, gd])
        else:
            torch.autograd.backward([outs[0], outs[1], outs[3]], [g, gd, ga])
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


def child(steps, mode):
    """rocprofv3 target: one mode, `steps` steps."""
    dev = torch.device("cuda:0")
    s, q, t = make()
    step = step_fn(s, q, t, mode, dev)
    for _ in range(steps):
        step()
    torch.cuda.synchronize()


def rocprof(steps, mode):
    out = tempfile.mkdtemp(prefix="depth_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "run", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--child", str(steps), "--mode", mode]
    subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
    stats = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    rows = {}
    if stats:
        for r in csv.DictReader(open(stats[0])):
            name = r.get("Name", "")
            if any(k in name for k in ("k_tile_order", "k_bwd_points", "k_sum_rows", "k_blend_bwd")):
                rows[name.split("(")[0]] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_grad_bench.json"))
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--mode", default="image", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.mode)
        return
    dev = torch.device("cuda:0")
    res = {"workload": "cfg3_headline", "step": "forward + backward of sum(g * image) [+ sum(gd * depth)] [+ sum(ga * alpha)]",
           "device": torch.cuda.get_device_name(0), "modes": {}}
    s, q, t = make()
    for mode in MODES:
        res["modes"][mode] = time_mode(s, q, t, mode, a.steps, a.warmup, dev)
    if a.rocprof:
        res["kernels_rocprofv3"] = {mode: rocprof(10, mode) for mode in MODES}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
