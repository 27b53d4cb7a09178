#!/usr/bin/env python3
"""Measure what it costs to put one training target on the device per step, at 1920x1088 and downsample factors 1, 2 and 4
(GaussianPointTrainer.py:103-121, 149-159), on cuda:0:
  (a) the reference's way as it can be run here: the f32 (3,H,W) image on the host, F.interpolate(antialias=True) on the CPU
      for a factor above 1, the crop, then the copy to the device -- from pageable memory (`.to(device)`) and through a pinned
      buffer (copy_ into it, then `.to(device)`: the DataLoader of the reference pins, its `.cuda()` blocks);
  (b) F.interpolate(antialias=True) and the crop on the device, from a resident f32 (3,H,W) image;
  (c) gs_image_resample from the resident uint8 image (targets.TargetStore.target).
and the whole training iteration of tools/bench_trainer_step.py (its fused_in_place leg, BASELINE config 3) with a resident
target as that tool has it, and with (a) and (c) producing the target every iteration, at factor 1.
Every leg is a host clock around a loop that ends in a synchronise (harness.wall_ms).  No ratio is asserted.

    python tools/bench_targets.py [--out profiles/targets_bench.json] [--steps N] [--warmup N] [--skip-iteration]
"""
import argparse

import harness as H
import numpy as np
import torch
import torch.nn.functional as F

from taichi_3d_gaussian_splatting_amd import CameraInfo, targets

DEV = "cuda:0"
HEIGHT, WIDTH = 1088, 1920
FACTORS = (1, 2, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--steps", type=int, help="timed calls of every leg (default: 20 on the CPU legs, 200 on the device legs, 50 iterations)")
    ap.add_argument("--warmup", type=int)
    ap.add_argument("--skip-iteration", action="store_true")
    a = ap.parse_args()
    H.require_gpu("bench_targets.py")

    def timeit(fn, n, warm):
        return round(H.wall_ms(fn, a.steps or n, warm if a.warmup is None else a.warmup), 4)

    u8 = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (HEIGHT, WIDTH, 3), dtype=np.uint8))
    host_f32 = u8.permute(2, 0, 1).float().div(255).contiguous()
    dev_f32 = host_f32.to(DEV)
    info = CameraInfo(torch.tensor([[1152.0, 0.0, 960.0], [0.0, 1152.0, 544.0], [0.0, 0.0, 1.0]]), HEIGHT, WIDTH, 0)
    store = targets.TargetStore([targets._pitched(u8, DEV)], torch.tensor([[0.0, 0.0, 0.0, 1.0]]), torch.zeros(1, 3), [info], DEV)

    def resized(image, f):
        h_full, w_full, h, w = targets.downsampled_geometry(HEIGHT, WIDTH, f)
        if f > 1:
            image = F.interpolate(image[None], size=(h_full, w_full), mode="bilinear", antialias=True, align_corners=False)[0]
        return image[:, :h, :w].contiguous()

    pinned = {f: torch.empty(resized(host_f32, f).shape, dtype=torch.float32).pin_memory() for f in FACTORS}

    def a_pageable(f):
        return resized(host_f32, f).to(DEV)

    def a_pinned(f):
        pinned[f].copy_(resized(host_f32, f))
        return pinned[f].to(DEV)

    legs = {}
    for f in FACTORS:
        h_full, w_full, h, w = targets.downsampled_geometry(HEIGHT, WIDTH, f)
        got, want = store.target(0, f)[0], resized(dev_f32, f)
        legs[f"factor_{f}"] = {
            "target": [3, h, w],
            "a_cpu_resize_and_copy_pageable_ms": timeit(lambda: a_pageable(f), 20, 3),
            "a_cpu_resize_and_copy_pinned_ms": timeit(lambda: a_pinned(f), 20, 3),
            "b_device_interpolate_from_f32_ms": timeit(lambda: resized(dev_f32, f), 200, 20),
            "c_kernel_from_uint8_ms": timeit(lambda: store.target(0, f), 200, 20),
            "max_abs_difference_b_c": float((got - want).abs().max()),
        }
    out = {
        "component": "one training target per step, 1920x1088, 1x MI355X",
        "cpu_threads": torch.get_num_threads(),
        "resident_bytes_per_image": {"uint8_hwc_16_byte_pitch": int(store.images[0].stride(0)) * HEIGHT, "f32_chw": dev_f32.numel() * 4},
        "per_target_ms": legs,
    }

    if not a.skip_iteration:
        from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast
        from taichi_3d_gaussian_splatting_amd.LossFunction import LossFunction
        from taichi_3d_gaussian_splatting_amd.optim import FusedAdam
        from taichi_3d_gaussian_splatting_amd.synthetic import make_scene, scene_input, view_pose
        s = make_scene("cfg3_headline")
        assert (s.height, s.width) == (HEIGHT, WIDTH)
        q, t = view_pose()
        inp = scene_input(s, q, t, DEV, requires_grad=True)
        pc, feat, mask = inp.point_cloud, inp.point_cloud_features, inp.point_invalid_mask
        rast = Rast(Rast.GaussianPointCloudRasterisationConfig(), backward_valid_point_hook=lambda x: None)
        of, op = FusedAdam([feat], lr=1e-3), FusedAdam([pc], lr=1e-5)
        loss_fn = LossFunction(LossFunction.LossFunctionConfig())

        def iteration(target):
            def it():
                of.zero_grad(); op.zero_grad()
                gt = target()
                img, _, _ = rast(inp)
                loss_fn(img.permute(2, 0, 1), gt, point_invalid_mask=mask, pointcloud_features=feat, clamp_predicted=True)[0].backward()
                of.step(); op.step()
            return it
        feeds = {"resident_target_as_bench_trainer_step": lambda: dev_f32, "a_pageable": lambda: a_pageable(1),
                 "a_pinned": lambda: a_pinned(1), "c_kernel_from_uint8": lambda: store.target(0, 1)[0]}
        out["training_iteration_ms_factor_1_cfg3"] = {name: timeit(iteration(feed), 50, 10) for name, feed in feeds.items()}
    H.write_json(out, a.out)


if __name__ == "__main__":
    main()
