"""Cost of the pose gradient (k_pose.hip) at cfg3_headline: forward + backward of sum(g * image) in three modes --
points only, points + pose, pose only -- at n_objects = 1 and 8 (points split into 8 objects with equal poses).
Device events time the steps (harness.per_call_ms); `--rocprof` adds one `rocprofv3 --kernel-trace --stats` run of a
child process for the per-kernel times.  Writes profiles/pose_grad_bench.json (or --out).

    python tools/bench_pose_grad.py [--workload cfg3_headline] [--steps 50] [--warmup 10] [--rocprof] [--out PATH]
"""
import argparse
import os

import harness as H
import numpy as np
import torch

from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast
from taichi_3d_gaussian_splatting_amd.synthetic import make_scene, scene_input, view_pose

MODES = {"points": (True, False), "points+pose": (True, True), "pose": (False, True)}


def make(workload, n_objects):
    s = make_scene(workload)
    q, t = view_pose()
    if n_objects > 1:
        s.point_object_id[:] = np.random.default_rng(1).integers(0, n_objects, s.point_object_id.shape[0]).astype(np.int32)
    q, t = np.repeat(q, n_objects, 0), np.repeat(t, n_objects, 0)
    return s, q, t


def step_fn(s, q, t, mode, dev):
    points, pose = MODES[mode]
    module = Rast(Rast.GaussianPointCloudRasterisationConfig())
    inp = scene_input(s, q, t, dev, requires_grad=points, pose=pose)
    leaves = (inp.point_cloud, inp.point_cloud_features, inp.q_pointcloud_camera, inp.t_pointcloud_camera)
    g = torch.full((s.height, s.width, 3), 1e-3, device=dev)

    def step():
        for x in leaves:
            x.grad = None
        image = module(inp)[0]
        image.backward(g)
    return step


def child(workload, steps):
    """rocprofv3 target: every mode at both object counts, `steps` steps each."""
    dev = torch.device("cuda:0")
    for n_objects in (1, 8):
        s, q, t = make(workload, n_objects)
        for mode in MODES:
            step = step_fn(s, q, t, mode, dev)
            for _ in range(steps):
                step()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3_headline")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--out", default=os.path.join(H.ROOT, "profiles", "pose_grad_bench.json"))
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    H.require_gpu("bench_pose_grad.py")
    if a.child:
        child(a.workload, a.child)
        return
    dev = torch.device("cuda:0")
    res = {"workload": a.workload, "step": "forward + backward of sum(g * image)", "device": torch.cuda.get_device_name(0),
           "modes": {}}
    for n_objects in (1, 8):
        s, q, t = make(a.workload, n_objects)
        for mode in MODES:
            m = H.summary(H.per_call_ms(step_fn(s, q, t, mode, dev), a.steps, a.warmup))
            del m["spread_ms"]          # the record keeps its four keys
            res["modes"][f"{mode}@kobj{n_objects}"] = m
    if a.rocprof:
        res["kernels_rocprofv3"] = H.rocprof_kernel_stats(
            [os.path.abspath(__file__), "--workload", a.workload, "--child", "10"],
            ("k_pose", "k_bwd_points", "k_sum_rows", "k_blend_bwd_tile"))
    H.write_json(res, a.out)


if __name__ == "__main__":
    main()
