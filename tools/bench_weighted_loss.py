#!/usr/bin/env python3
"""Measure what per-pixel weights cost (include/gs_loss_weighted.h, include/gs_targets_rgba.h), on cuda:0:
  loss      forward + backward at 1920x1088 and 976x544, the predicted image in the rasteriser's interleaved (H,W,3) layout
            (clamped inside the kernels) against a planar (3,H,W) target: the weighted call, the unweighted call on the same
            images, and a torch restatement of the weighted definition (conv2d + autograd) on the same device;
  target    TargetStore.target(i, f, with_weight=True) against target(i, f) from the same resident uint8 RGBA image;
  iteration a whole training iteration (tools/bench_trainer_step.py's fused_in_place leg plus the target's launch) at BASELINE
            config 3, with and without weights.
Each comparison alternates its legs in one process (harness.alternate: every leg warmed, then `repeats` rounds of one timed
window per leg, a window being `--steps` calls between two device events).  No ratio is asserted.  The unweighted kernels are
the baseline; `--rocprof` adds one `rocprofv3 --kernel-trace --stats` run of a child process per loss leg and size for the loss
kernels' own times (the host side of a call is a large part of the windows above); the weighted forward reads one more f32 plane per channel-block and the backward one more, so a cost of more
than about a quarter over the unweighted time is a finding the notes must explain.

    python tools/bench_weighted_loss.py [--out profiles/weighted_loss_bench.json] [--steps N] [--warmup N] [--repeats N]
                                        [--sizes 1088x1920,544x976] [--workload cfg3_headline] [--skip-iteration] [--rocprof]
"""
import argparse
import os

import harness as H
import numpy as np
import torch
import torch.nn.functional as F

from taichi_3d_gaussian_splatting_amd import CameraInfo, targets
from taichi_3d_gaussian_splatting_amd.LossFunction import LossFunction

DEV = "cuda:0"
SIZES = "1088x1920,544x976"


def torch_weighted_loss(pred_hwc, gt, weight, lam=0.2):
    """the definition of gs_loss_weighted.h in torch ops, f32: clamp, weighted L1, centre-weighted SSIM"""
    x = torch.clamp(pred_hwc, 0, 1).permute(2, 0, 1)
    w = torch.where(weight > 0, weight, torch.zeros_like(weight))
    v = w[5:-5, 5:-5]
    coords = torch.arange(11, dtype=x.dtype, device=x.device) - 5
    g = torch.exp(-(coords ** 2) / (2 * 1.5 ** 2))
    g = (g / g.sum()).reshape(1, 1, 1, 11).repeat(3, 1, 1, 1)
    gf = lambda t: F.conv2d(F.conv2d(t, g.transpose(2, 3), groups=3), g, groups=3)
    X, Y = x[None], gt[None]
    mu1, mu2 = gf(X), gf(Y)
    s1, s2, s12 = gf(X * X) - mu1 ** 2, gf(Y * Y) - mu2 ** 2, gf(X * Y) - mu1 * mu2
    ssim_map = ((2 * mu1 * mu2 + 1e-4) / (mu1 ** 2 + mu2 ** 2 + 1e-4)) * ((2 * s12 + 9e-4) / (s1 + s2 + 9e-4))
    l1 = (w * (x - gt).abs()).sum() / (3 * w.sum())
    return (1 - lam) * l1 + lam * (1 - (v * ssim_map[0]).sum() / (3 * v.sum()))


def soft_mask(h, w, device):
    """a foreground ellipse with a soft rim and a hole: about half the picture, weights in [0, 1]"""
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, h, device=device), torch.linspace(-1, 1, w, device=device), indexing="ij")
    r = (xx / 0.85) ** 2 + (yy / 0.8) ** 2
    m = torch.clamp((1.0 - r) * 12, 0, 1)
    m[(xx - 0.2).abs() + (yy + 0.1).abs() < 0.15] = 0.0
    return m.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--steps", type=int, default=50, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=100, help="untimed calls of every leg")
    ap.add_argument("--repeats", type=int, default=5, help="alternating rounds")
    ap.add_argument("--sizes", default=SIZES, help="HxW,HxW of the loss and target legs")
    ap.add_argument("--workload", default="cfg3_headline")
    ap.add_argument("--skip-iteration", action="store_true")
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--child", choices=("weighted", "unweighted"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    H.require_gpu("bench_weighted_loss.py")
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    if a.child:                 # rocprofv3 target: one loss leg at the first size, that many calls
        h, w = sizes[0]
        gt = torch.rand(3, h, w, device=DEV)
        raw = torch.rand(h, w, 3, device=DEV) * 1.2 - 0.1
        weight = soft_mask(h, w, DEV) if a.child == "weighted" else None
        lf = LossFunction(LossFunction.LossFunctionConfig(enable_regularization=False))
        for _ in range(a.steps):
            p = raw.detach().requires_grad_(True)
            lf(p.permute(2, 0, 1), gt, clamp_predicted=True, pixel_weight=weight)[0].backward()
        torch.cuda.synchronize()
        return
    lf = LossFunction(LossFunction.LossFunctionConfig(enable_regularization=False))
    gen = torch.Generator(device=DEV).manual_seed(0)
    out = {"component": "per-pixel weights: fused loss, target and training iteration, 1x MI355X",
           "method": f"harness.alternate: {a.warmup} warm calls per leg, {a.repeats} rounds of one {a.steps}-call window per leg between device events",
           "loss_fwd_bwd_ms": {}, "target_ms": {}, "notes": []}

    for (h, w) in sizes:
        gt = torch.rand(3, h, w, device=DEV, generator=gen)
        raw = (gt.permute(1, 2, 0) * 1.2 - 0.1 + 0.1 * torch.randn(h, w, 3, device=DEV, generator=gen)).contiguous()
        weight = soft_mask(h, w, DEV)

        def weighted():
            p = raw.detach().requires_grad_(True)
            lf(p.permute(2, 0, 1), gt, clamp_predicted=True, pixel_weight=weight)[0].backward()

        def unweighted():
            p = raw.detach().requires_grad_(True)
            lf(p.permute(2, 0, 1), gt, clamp_predicted=True)[0].backward()

        def torch_restatement():
            p = raw.detach().requires_grad_(True)
            torch_weighted_loss(p, gt, weight).backward()
        p = raw.detach().requires_grad_(True)
        fused = lf(p.permute(2, 0, 1), gt, clamp_predicted=True, pixel_weight=weight)[0]
        rec = H.alternate({"weighted_fused": weighted, "unweighted_fused": unweighted, "weighted_torch_conv2d_autograd": torch_restatement},
                          a.steps, a.warmup, a.repeats)
        rec["weighted_over_unweighted"] = round(rec["weighted_fused"]["median_ms"] / rec["unweighted_fused"]["median_ms"], 4)
        rec["torch_over_weighted"] = round(rec["weighted_torch_conv2d_autograd"]["median_ms"] / rec["weighted_fused"]["median_ms"], 3)
        rec["abs_difference_fused_torch"] = abs(float(fused) - float(torch_weighted_loss(raw, gt, weight)))
        rec["weighted_share_of_pixels"] = round(float((weight > 0).float().mean()), 4)
        out["loss_fwd_bwd_ms"][f"{h}x{w}"] = rec

        # the target: the same picture resident as uint8 RGBA, at the size itself (factor 1) and at half of it
        u8 = torch.cat([(gt.permute(1, 2, 0) * 255).round().to(torch.uint8), (weight * 255).round().to(torch.uint8)[..., None]], dim=2).cpu()
        info = CameraInfo(torch.tensor([[1152.0, 0.0, w / 2], [0.0, 1152.0, h / 2], [0.0, 0.0, 1.0]]), h - h % 16, w - w % 16, 0)
        store = targets.TargetStore([targets._pitched(u8, DEV)], torch.tensor([[0.0, 0.0, 0.0, 1.0]]), torch.zeros(1, 3), [info], DEV)
        for f in (1, 2):
            plain = store.target(0, f)[0].clone()
            both = store.target(0, f, with_weight=True)
            assert torch.equal(both[0], plain)
            rec = H.alternate({"target_with_weight": lambda: store.target(0, f, with_weight=True), "target": lambda: store.target(0, f)},
                              a.steps, a.warmup, a.repeats)
            rec["with_weight_over_plain"] = round(rec["target_with_weight"]["median_ms"] / rec["target"]["median_ms"], 4)
            rec["output"] = [4] + list(both[4].shape)
            out["target_ms"][f"{h}x{w}_factor_{f}"] = rec

    if a.skip_iteration:
        out["training_iteration_ms"] = "not measured"
    else:
        from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast
        from taichi_3d_gaussian_splatting_amd.optim import FusedAdam
        from taichi_3d_gaussian_splatting_amd.synthetic import make_scene, scene_input, view_pose
        s = make_scene(a.workload)
        q, t = view_pose()
        inp = scene_input(s, q, t, DEV, requires_grad=True)
        pc, feat, mask = inp.point_cloud, inp.point_cloud_features, inp.point_invalid_mask
        rast = Rast(Rast.GaussianPointCloudRasterisationConfig(), backward_valid_point_hook=lambda x: None)
        of, op = FusedAdam([feat], lr=1e-3), FusedAdam([pc], lr=1e-5)
        loss_fn = LossFunction(LossFunction.LossFunctionConfig())
        rgba = torch.cat([torch.from_numpy(np.random.default_rng(0).integers(0, 256, (s.height, s.width, 3), dtype=np.uint8)),
                          (soft_mask(s.height, s.width, "cpu") * 255).round().to(torch.uint8)[..., None]], dim=2)
        info = CameraInfo(torch.tensor(s.camera_intrinsics), s.height - s.height % 16, s.width - s.width % 16, 0)
        assert (info.camera_height, info.camera_width) == (s.height, s.width), "the workload's size must be a multiple of 16"
        store = targets.TargetStore([targets._pitched(rgba, DEV)], torch.tensor([[0.0, 0.0, 0.0, 1.0]]), torch.zeros(1, 3), [info], DEV)

        def iteration(with_weight):
            def it():
                of.zero_grad(); op.zero_grad()
                got = store.target(0, 1, with_weight=with_weight)
                img, _, _ = rast(inp)
                loss_fn(img.permute(2, 0, 1), got[0], point_invalid_mask=mask, pointcloud_features=feat, clamp_predicted=True,
                        pixel_weight=got[4] if with_weight else None)[0].backward()
                of.step(); op.step()
            return it
        rec = H.alternate({"with_weights": iteration(True), "without_weights": iteration(False)}, max(a.steps // 2, 1), a.warmup, a.repeats)
        rec["with_over_without"] = round(rec["with_weights"]["median_ms"] / rec["without_weights"]["median_ms"], 4)
        rec["workload"] = a.workload
        out["training_iteration_ms"] = rec

    out["loss_kernels_rocprofv3"] = "not measured"
    if a.rocprof:
        out["loss_kernels_rocprofv3"] = {f"{h}x{w}": {leg: H.rocprof_kernel_stats(
            [os.path.abspath(__file__), "--sizes", f"{h}x{w}", "--steps", "20", "--child", leg], ("k_loss_",), seconds=120)
            for leg in ("weighted", "unweighted")} for (h, w) in sizes}
        for key, legs_ in out["loss_kernels_rocprofv3"].items():
            us = {leg: round(sum(r["avg_us"] for r in rows.values()), 2) for leg, rows in legs_.items()}
            legs_["sum_of_kernel_averages_us"] = us
    for key, rec in out["loss_fwd_bwd_ms"].items():
        if rec["weighted_over_unweighted"] > 1.25:
            out["notes"].append(f"loss {key}: the weighted call takes {rec['weighted_over_unweighted']}x the unweighted one, over the quarter "
                                "expected from one more f32 plane per channel-block: to be explained before the number is relied on")
    for key, rec in out["target_ms"].items():
        if rec["with_weight_over_plain"] > 1.25:
            out["notes"].append(f"target {key}: {rec['with_weight_over_plain']}x the three-plane call; it stores four f32 planes instead of "
                                "three (4/3 of the bytes written, the larger part of what the launch moves from a uint8 source)")
    def legs(doc, path=()):
        if isinstance(doc, dict) and "windows_ms" in doc:
            yield "/".join(path), doc
        elif isinstance(doc, dict):
            for k, v in doc.items():
                yield from legs(v, path + (k,))
    for name, leg in legs(out):
        if leg["max_ms"] > 1.5 * leg["min_ms"]:
            out["notes"].append(f"{name}: its windows span {leg['min_ms']} to {leg['max_ms']} ms ({leg['windows_ms']}): more than one "
                                "regime in one leg, so its median and the ratios made from it are not a steady-state figure")
    medians = [rec["unweighted_fused"]["median_ms"] for rec in out["loss_fwd_bwd_ms"].values()]
    if len(medians) > 1 and max(medians) < 1.15 * min(medians):
        out["notes"].append("loss: the unweighted call takes the same time at every size measured (within 15 %), so these windows are "
                            "bound by the call's host side (autograd node, two library calls, three launches) and the ratios say "
                            "what a caller pays per call, not what the kernels take; per-kernel times: not measured")
    H.write_json(out, a.out)


if __name__ == "__main__":
    main()
