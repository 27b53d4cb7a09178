"""Cost of the differentiable depth / accumulated alpha (gs_backward_ex) at cfg3_headline: forward + backward in three modes --
image only (gs_backward, today's path), image + depth (config.differentiable_depth) and image + depth + alpha
(forward(..., return_accumulated_alpha=True)).  Device events time the steps (harness.per_call_ms); `--rocprof` adds one
`rocprofv3 --kernel-trace --stats` run of a child process per mode for the per-kernel times (the AUX instantiations show up
under their template arguments).  Writes profiles/depth_grad_bench.json (or --out).

    python tools/bench_depth_grad.py [--workload cfg3_headline] [--steps 50] [--warmup 10] [--rocprof] [--out PATH]
"""
import argparse
import os

import harness as H
import torch

from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast
from taichi_3d_gaussian_splatting_amd.synthetic import make_scene, scene_input, view_pose

MODES = ["image", "image+depth", "image+depth+alpha"]


def step_fn(s, q, t, mode, dev):
    cfg = Rast.GaussianPointCloudRasterisationConfig()
    cfg.differentiable_depth = mode != "image"
    module = Rast(cfg)
    alpha = mode.endswith("alpha")
    inp = scene_input(s, q, t, dev, requires_grad=True)
    g = torch.full((s.height, s.width, 3), 1e-3, device=dev)
    gd = torch.full((s.height, s.width), 1e-3, device=dev)
    ga = torch.full((s.height, s.width), -1e-3, device=dev)

    def step():
        inp.point_cloud.grad = inp.point_cloud_features.grad = None
        outs = module(inp, return_accumulated_alpha=alpha)
        if mode == "image":
            outs[0].backward(g)
        elif mode == "image+depth":
            torch.autograd.backward([outs[0], outs[1]], [g, gd])
        else:
            torch.autograd.backward([outs[0], outs[1], outs[3]], [g, gd, ga])
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3_headline")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--out", default=os.path.join(H.ROOT, "profiles", "depth_grad_bench.json"))
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--mode", default="image", help=argparse.SUPPRESS)
    a = ap.parse_args()
    H.require_gpu("bench_depth_grad.py")
    dev = torch.device("cuda:0")
    s = make_scene(a.workload)
    q, t = view_pose()
    if a.child:                 # rocprofv3 target: one mode, that many steps
        step = step_fn(s, q, t, a.mode, dev)
        for _ in range(a.child):
            step()
        torch.cuda.synchronize()
        return
    res = {"workload": a.workload, "step": "forward + backward of sum(g * image) [+ sum(gd * depth)] [+ sum(ga * alpha)]",
           "device": torch.cuda.get_device_name(0), "modes": {}}
    for mode in MODES:
        m = H.summary(H.per_call_ms(step_fn(s, q, t, mode, dev), a.steps, a.warmup))
        del m["spread_ms"]          # the record keeps its four keys
        res["modes"][mode] = m
    if a.rocprof:
        res["kernels_rocprofv3"] = {mode: H.rocprof_kernel_stats(
            [os.path.abspath(__file__), "--workload", a.workload, "--child", "10", "--mode", mode],
            ("k_tile_order", "k_bwd_points", "k_sum_rows", "k_blend_bwd")) for mode in MODES}
    H.write_json(res, a.out)


if __name__ == "__main__":
    main()
