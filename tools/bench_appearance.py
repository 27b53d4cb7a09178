#!/usr/bin/env python3
"""Measure exposure compensation (include/gs_appearance.h, appearance.py), on cuda:0:
  calls      at every --sizes image: gs_appearance_apply, gs_appearance_backward (both gradients) and gs_appearance_moments on
             the rasteriser's interleaved layout (the target of the moments planar, as a photograph is), beside the same
             formulas written in torch operations on the same device: apply as one addmm over the (H W, 3) pixels, the backward
             as the selection, two matmuls and a sum, the moments as float64 matmuls.  Every call of a leg takes the next of
             enough buffer sets to hold more than --footprint-mb, so that the images come from HBM and not from the 256 MB
             Infinity Cache; each call's bytes stand beside the time they would take at the 6.3 TB/s a float4 copy reaches on
             this part (hbm_floor_ms).  A window holds the host's share of a call too; with --rocprof the kernels' own time
             (device_us: the image pass and, for the two calls with sums, its finishing kernel) is taken from a rocprofv3
             kernel trace of a child process that makes the same calls.
  iteration  a whole training iteration at --workload (tools/bench_trainer_step.py's fused_in_place leg) with
             appearance "affine" -- apply in front of the loss, its backward behind it, the row's Adam step -- beside "none".
Each comparison alternates its legs in one process (harness.alternate: every leg warmed, then `repeats` rounds of one timed
window per leg, a window being `--steps` calls between two device events).  No ratio is asserted.

    python tools/bench_appearance.py [--out profiles/appearance_bench.json] [--sizes 1920x1088,976x544] [--steps N] [--warmup N]
                                     [--repeats N] [--workload cfg3_headline] [--skip-iteration] [--rocprof]
"""
import argparse
import os

import harness as H
import torch

from taichi_3d_gaussian_splatting_amd import appearance

DEV = "cuda:0"
SIZES = "1920x1088,976x544"
HBM_BYTES_PER_S = 6.3e12            # achievable: a float4 copy
KEYS = ("component", "method", "calls_ms", "training_iteration_ms", "notes")


class Ring:
    """n sets of tensors made by make(i); next() walks them"""

    def __init__(self, make, n):
        self.sets, self.i = [make(i) for i in range(n)], -1

    def next(self):
        self.i = (self.i + 1) % len(self.sets)
        return self.sets[self.i]


def torch_apply(x_hw3, M):
    A, b = M.view(3, 4)[:, :3], M.view(3, 4)[:, 3]
    return torch.addmm(b, x_hw3.view(-1, 3), A.t()).view_as(x_hw3)


def torch_backward(x_hw3, g_hw3, M):
    A = M.view(3, 4)[:, :3]
    g, x = g_hw3.view(-1, 3), x_hw3.view(-1, 3)
    selected = (g != 0).any(dim=1, keepdim=True)
    x = torch.where(selected, x, torch.zeros_like(x))
    return g @ A, torch.cat([g.t() @ x, g.sum(0)[:, None]], dim=1)


def torch_moments(x_hw3, y_3hw, w_hw):
    x, y = x_hw3.view(-1, 3).double(), y_3hw.reshape(3, -1).double()
    w = torch.where(w_hw > 0, w_hw, torch.zeros_like(w_hw)).reshape(-1, 1).double()
    u = torch.cat([x, torch.ones_like(w)], dim=1)
    wu = torch.where(w > 0, w * u, torch.zeros_like(u))
    return wu.t() @ u, y @ wu, w.sum()


def call_legs(Hh, W, M, gen, footprint_mb):
    """yields (name, the library's call, the torch restatement, its name, bytes the kernel has to move) of the three calls, each
    over a ring of buffer sets that is freed before the next is made"""
    image_bytes = 3 * Hh * W * 4

    def sets(images):
        return max(2, -(-footprint_mb * 10 ** 6 // (images * image_bytes)))

    def image(i):
        return torch.rand(Hh, W, 3, device=DEV, generator=gen)

    ring = Ring(lambda i: (image(i), torch.empty(Hh, W, 3, device=DEV)), sets(2))

    def hip_apply():
        x, c = ring.next()
        appearance.apply_forward(x.permute(2, 0, 1), M, out=c.permute(2, 0, 1))
    yield "apply", hip_apply, lambda: torch_apply(ring.next()[0], M), "torch", 2 * image_bytes
    del ring
    torch.cuda.empty_cache()

    grad_transform = torch.empty(12, device=DEV)
    ring = Ring(lambda i: (image(i), image(i) - 0.5, torch.empty(Hh, W, 3, device=DEV)), sets(3))

    def hip_backward():
        x, g, gi = ring.next()
        appearance.apply_backward(x.permute(2, 0, 1), g.permute(2, 0, 1), M, grad_image=gi.permute(2, 0, 1), grad_transform=grad_transform)
    yield "backward", hip_backward, lambda: torch_backward(*ring.next()[:2], M), "torch", 3 * image_bytes
    del ring
    torch.cuda.empty_cache()

    ring = Ring(lambda i: (image(i), torch.rand(3, Hh, W, device=DEV, generator=gen), torch.rand(Hh, W, device=DEV, generator=gen) - 0.2),
                sets(2))

    def hip_moments():
        x, y, w = ring.next()
        appearance.moments(x.permute(2, 0, 1), y, w)
    yield "moments", hip_moments, lambda: torch_moments(*ring.next()), "torch_float64", 2 * image_bytes + image_bytes // 3
    del ring
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--sizes", default=SIZES, help="WxH of the images, comma separated")
    ap.add_argument("--steps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=20, help="untimed calls of every leg")
    ap.add_argument("--repeats", type=int, default=5, help="alternating rounds")
    ap.add_argument("--footprint-mb", type=int, default=600, help="bytes the buffer sets of a leg hold together, at least")
    ap.add_argument("--workload", default="cfg3_headline")
    ap.add_argument("--skip-iteration", action="store_true")
    ap.add_argument("--rocprof", action="store_true", help="the kernels' own time by a rocprofv3 kernel trace of a child process")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    H.require_gpu("bench_appearance.py")
    out = {"component": "exposure compensation: apply, backward, moments and training iteration, 1x MI355X",
           "method": f"harness.alternate: {a.warmup} warm calls per leg, {a.repeats} rounds of one {a.steps}-call window per leg between device "
                     f"events; every call on the next of enough buffer sets to hold {a.footprint_mb} MB",
           "calls_ms": {}, "notes": []}
    gen = torch.Generator(device=DEV).manual_seed(0)
    M = torch.tensor(appearance.IDENTITY, device=DEV) + 0.05 * torch.randn(12, device=DEV, generator=gen)
    if a.child:                 # rocprofv3 target: the three calls at the first size, warm-up included in the averages' calls
        W, Hh = (int(v) for v in a.sizes.split(",")[0].lower().split("x"))
        for _, hip, _, _, _ in call_legs(Hh, W, M, gen, a.footprint_mb):
            for _ in range(a.warmup + a.steps):
                hip()
            torch.cuda.synchronize()
        return
    for size in a.sizes.split(","):
        W, Hh = (int(v) for v in size.lower().split("x"))
        rec = {"height": Hh, "width": W, "image_mb": round(3 * Hh * W * 4 / 1e6, 3)}
        for name, hip, tch, other, nbytes in call_legs(Hh, W, M, gen, a.footprint_mb):
            leg = H.alternate({"hip": hip, other: tch}, a.steps, a.warmup, a.repeats)
            leg["bytes"] = nbytes
            leg["hbm_floor_ms"] = round(nbytes / HBM_BYTES_PER_S * 1e3, 5)
            leg["torch_over_hip"] = round(leg[other]["median_ms"] / leg["hip"]["median_ms"], 3)
            rec[name] = leg
        if a.rocprof:
            # the windows above hold the host's share of a call too (two launches cost more host time than these kernels run):
            # the kernels' own time comes from a kernel trace of a child process that makes the same calls
            rows = H.rocprof_kernel_stats([os.path.abspath(__file__), "--sizes", size, "--steps", str(a.steps * a.repeats), "--warmup",
                                           str(a.warmup), "--footprint-mb", str(a.footprint_mb), "--child"], ("k_appearance_",), seconds=240)
            rec["kernels_rocprofv3"] = rows

            def us(*parts):
                return round(sum(r["avg_us"] for k, r in rows.items() if any(part in k for part in parts)), 3)
            device = {"apply": us("k_appearance_apply"), "backward": us("k_appearance_backward", "finish<float"),
                      "moments": us("k_appearance_moments", "finish<double")}
            for name, value in device.items():
                rec[name]["device_us"] = value
                rec[name]["device_over_hbm_floor"] = round(value / (rec[name]["hbm_floor_ms"] * 1e3), 3)
        out["calls_ms"][f"{W}x{Hh}"] = rec

    if a.skip_iteration:
        out["training_iteration_ms"] = "not measured"
    else:
        from taichi_3d_gaussian_splatting_amd import GaussianPointAdaptiveController, GaussianPointCloudRasterisation as Rast
        from taichi_3d_gaussian_splatting_amd.LossFunction import LossFunction
        from taichi_3d_gaussian_splatting_amd.optim import FusedAdam
        from taichi_3d_gaussian_splatting_amd.synthetic import make_scene, scene_input, view_pose
        s = make_scene(a.workload)
        q, t = view_pose()
        inp = scene_input(s, q, t, DEV, requires_grad=True)
        controller_config = GaussianPointAdaptiveController.GaussianPointAdaptiveControllerConfig()
        controller_config.num_iterations_warm_up = 10 ** 9
        controller = GaussianPointAdaptiveController(
            config=controller_config, maintained_parameters=GaussianPointAdaptiveController.GaussianPointAdaptiveControllerMaintainedParameters(
                pointcloud=inp.point_cloud, pointcloud_features=inp.point_cloud_features, point_invalid_mask=inp.point_invalid_mask,
                point_object_id=inp.point_object_id), seed=0)
        rast = Rast(Rast.GaussianPointCloudRasterisationConfig(), backward_valid_point_hook=controller.update)
        of, op = FusedAdam([inp.point_cloud_features], lr=1e-3), FusedAdam([inp.point_cloud], lr=1e-5)
        table = appearance.AppearanceTable(8, DEV, appearance.AppearanceConfig(num_iterations=30_000))
        loss_fn = LossFunction(LossFunction.LossFunctionConfig())
        gt = torch.rand(3, s.height, s.width, device=DEV, generator=gen)
        count = [0]

        def iteration(mode):
            def it():
                count[0] += 1
                view = count[0] % table.num_views
                of.zero_grad(); op.zero_grad()
                img = rast(inp)[0].permute(2, 0, 1)
                if mode == "affine":
                    img = appearance.apply(img, table.row(view))
                loss_fn(img, gt, point_invalid_mask=inp.point_invalid_mask, pointcloud_features=inp.point_cloud_features,
                        clamp_predicted=True)[0].backward()
                of.step(); op.step()
                if mode == "affine":
                    table.step(view, count[0])
                controller.refinement()
            return it
        rec = H.alternate({"affine": iteration("affine"), "none": iteration("none")}, a.steps, a.warmup, a.repeats)
        rec["affine_minus_none_ms"] = round(rec["affine"]["median_ms"] - rec["none"]["median_ms"], 5)
        rec["affine_over_none"] = round(rec["affine"]["median_ms"] / rec["none"]["median_ms"], 4)
        rec["workload"], rec["height"], rec["width"] = a.workload, s.height, s.width
        out["training_iteration_ms"] = rec

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
    assert set(out) == set(KEYS)
    H.write_json(out, a.out)


if __name__ == "__main__":
    main()
