#!/usr/bin/env python3
"""Measure the pieces either side of the operator at BASELINE config 3 on cuda:0:
L1+SSIM loss forward+backward and the two Adam updates, libgsrast's fused kernels against the torch ops the
reference would run (conv2d-based SSIM restated from pytorch_msssim + autograd; torch.optim.Adam), and a whole
training iteration (GaussianPointTrainer.py:145-184 without data loading / logging).  Every leg is a host clock around a
loop that ends in a synchronise (harness.wall_ms): 10 + 50 calls of the loss and Adam legs, 20 + 100 iterations, unless
--warmup / --steps say otherwise.  Prints one JSON line (and writes it to --out).

    python tools/bench_trainer_step.py [--workload cfg3_headline] [--steps N] [--warmup N] [--out PATH]
    ... --only-iteration fused|fused_in_place|torch [--steps N]   for rocprofv3 --kernel-trace --stats: that iteration's launches alone
    ... --only-loss-chw | --only-loss-hwc                         the same for the loss kernels alone, one layout
"""
import argparse

import harness as H
import torch
import torch.nn.functional as F

from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast
from taichi_3d_gaussian_splatting_amd.LossFunction import LossFunction
from taichi_3d_gaussian_splatting_amd.optim import FusedAdam
from taichi_3d_gaussian_splatting_amd.synthetic import make_scene, scene_input, view_pose

DEV = "cuda:0"
ITERATIONS = {"fused_in_place": ("fused_loss_and_adam_image_in_place", True, True), "fused": ("fused_loss_and_adam", True, False),
              "torch": ("torch_loss_and_adam", False, False)}


def torch_loss(pred, gt, lam=0.2):
    coords = torch.arange(11, dtype=pred.dtype, device=pred.device) - 5
    g = torch.exp(-(coords ** 2) / (2 * 1.5 ** 2))
    g = (g / g.sum()).reshape(1, 1, 1, 11).repeat(3, 1, 1, 1)
    gf = lambda t: F.conv2d(F.conv2d(t, g.transpose(2, 3), groups=3), g, groups=3)
    X, Y = pred[None], gt[None]
    mu1, mu2 = gf(X), gf(Y)
    s1, s2, s12 = gf(X * X) - mu1 ** 2, gf(Y * Y) - mu2 ** 2, gf(X * Y) - mu1 * mu2
    ssim_map = ((2 * mu1 * mu2 + 1e-4) / (mu1 ** 2 + mu2 ** 2 + 1e-4)) * ((2 * s12 + 9e-4) / (s1 + s2 + 9e-4))
    return (1 - lam) * (pred - gt).abs().mean() + lam * (1 - ssim_map.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3_headline")
    ap.add_argument("--steps", type=int, help="timed calls of every leg")
    ap.add_argument("--warmup", type=int, help="untimed calls before every leg")
    ap.add_argument("--out", help="also write the line there")
    ap.add_argument("--only-iteration", choices=tuple(ITERATIONS))
    ap.add_argument("--only-fused-iteration", dest="only_iteration", action="store_const", const="fused_in_place",
                    help="the same as --only-iteration fused_in_place")
    ap.add_argument("--only-loss-chw", action="store_true")
    ap.add_argument("--only-loss-hwc", action="store_true")
    a = ap.parse_args()
    H.require_gpu("bench_trainer_step.py")

    def timeit(fn, n=50, warm=10):
        return H.wall_ms(fn, a.steps or n, warm if a.warmup is None else a.warmup)
    s = make_scene(a.workload)
    q, t = view_pose()
    gt = torch.rand(3, s.height, s.width, device=DEV)
    pred0 = torch.rand(3, s.height, s.width, device=DEV)
    lf = LossFunction(LossFunction.LossFunctionConfig(enable_regularization=False))

    def loss_fused():
        p = pred0.detach().requires_grad_(True)
        lf(p, gt)[0].backward()

    def loss_torch():
        p = pred0.detach().requires_grad_(True)
        torch_loss(p, gt).backward()

    N = s.point_cloud.shape[0]
    feat_a, pc_a = torch.randn(N, 56, device=DEV, requires_grad=True), torch.randn(N, 3, device=DEV, requires_grad=True)
    feat_a.grad, pc_a.grad = torch.randn_like(feat_a), torch.randn_like(pc_a)
    fa, fp = FusedAdam([feat_a], lr=1e-3), FusedAdam([pc_a], lr=1e-5)
    ta, tp = torch.optim.Adam([feat_a], lr=1e-3), torch.optim.Adam([pc_a], lr=1e-5)

    def make_iteration(fused, in_place=False):
        inp = scene_input(s, q, t, DEV, requires_grad=True)
        pc, feat, mask = inp.point_cloud, inp.point_cloud_features, inp.point_invalid_mask
        rast = Rast(Rast.GaussianPointCloudRasterisationConfig(), backward_valid_point_hook=lambda x: None)
        if fused:
            of, op = FusedAdam([feat], lr=1e-3), FusedAdam([pc], lr=1e-5)
            loss_fn = LossFunction(LossFunction.LossFunctionConfig())
        else:
            of, op = torch.optim.Adam([feat], lr=1e-3), torch.optim.Adam([pc], lr=1e-5)
            loss_fn = None

        def it():
            of.zero_grad(); op.zero_grad()
            img, _, _ = rast(inp)
            if in_place:        # the (H,W,3) image read where it lies, clamped inside the loss kernels
                L = loss_fn(img.permute(2, 0, 1), gt, point_invalid_mask=mask, pointcloud_features=feat, clamp_predicted=True)[0]
                L.backward()
                of.step(); op.step()
                return
            img = torch.clamp(img, 0, 1).permute(2, 0, 1)               # GaussianPointTrainer.py:173-176 as written
            if fused:
                L = loss_fn(img, gt, point_invalid_mask=mask, pointcloud_features=feat)[0]
            else:
                L = torch_loss(img, gt) + 2 * torch.norm(torch.exp(feat[mask == 0, 4:7]), dim=1).mean()
            L.backward()
            of.step(); op.step()
        return it

    if a.only_loss_chw or a.only_loss_hwc:
        flag, hwc = ("--only-loss-hwc", True) if a.only_loss_hwc else ("--only-loss-chw", False)
        raw = torch.rand(s.height, s.width, 3, device=DEV) * 1.4 - 0.2

        def loss_only():
            if hwc:
                p = raw.detach().requires_grad_(True)
                lf(p.permute(2, 0, 1), gt, clamp_predicted=True)[0].backward()
            else:
                loss_fused()
        H.write_json({flag: round(timeit(loss_only, n=100, warm=20), 4)}, a.out, indent=None)
        return

    def iteration_ms(which):
        key, fused, in_place = ITERATIONS[which]
        return key, round(timeit(make_iteration(fused, in_place), n=100, warm=20), 4)
    if a.only_iteration:
        H.write_json({"training_iteration_ms": dict([iteration_ms(a.only_iteration)])}, a.out, indent=None)
        return
    out = {
        "component": "trainer step around the rasteriser (SURVEY 8f-1), %s, 1x MI355X" % (
            "config 3" if a.workload == "cfg3_headline" else a.workload),
        "loss_fwd_bwd_ms": {"fused_gs_loss_l1_ssim": round(timeit(loss_fused), 4), "torch_conv2d_autograd": round(timeit(loss_torch), 4)},
        "adam_two_tensors_ms": {"fused_gs_adam_step": round(timeit(lambda: (fa.step(), fp.step())), 4),
                                "torch_optim_adam": round(timeit(lambda: (ta.step(), tp.step())), 4)},
        "training_iteration_ms": dict(iteration_ms(which) for which in ITERATIONS),
    }
    out["training_iterations_per_s"] = {k: round(1e3 / v, 1) for k, v in out["training_iteration_ms"].items()}
    H.write_json(out, a.out, indent=None)


if __name__ == "__main__":
    main()
