"""cProfile of the Python side of one fwd+bwd step at cfg3_headline (or the workload given): 30 untimed and 300 profiled
steps, the 28 entries with the largest cumulative time.  `python tools/host_profile.py [workload]` (GPU)"""
import argparse
import cProfile
import pstats

import harness as H
import torch

from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast
from taichi_3d_gaussian_splatting_amd.synthetic import make_scene, scene_input, view_pose


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="cfg3_headline")
    wl = ap.parse_args().workload
    H.require_gpu("host_profile.py")
    dev = torch.device("cuda", 0)
    s = make_scene(wl)
    inp = scene_input(s, *view_pose(), dev, requires_grad=True)
    module = Rast(Rast.GaussianPointCloudRasterisationConfig(), backward_valid_point_hook=lambda p: None)
    minus_one = torch.full((s.height, s.width, 3), -1.0, device=dev)

    def step():
        inp.point_cloud.grad = inp.point_cloud_features.grad = None
        image, _, _ = module(inp)
        g = torch.add(minus_one, image.detach(), alpha=2.0)
        image.backward(g)
    for _ in range(30):
        step()
    torch.cuda.synchronize()
    pr = cProfile.Profile()
    pr.enable()
    for _ in range(300):
        step()
    pr.disable()
    torch.cuda.synchronize()
    pstats.Stats(pr).sort_stats("cumulative").print_stats(28)


if __name__ == "__main__":
    main()
