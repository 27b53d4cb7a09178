#!/usr/bin/env python3
"""Measure the bilateral grids (include/gs_bilateral.h, bilateral.py), on cuda:0:
  calls      at every --sizes image, with a --grid grid: gs_bilateral_slice, gs_bilateral_slice_backward with both outputs and
             with the image's alone, on the rasteriser's interleaved layout, and gs_bilateral_tv with its gradient -- beside
             the same formulas in torch operations on the same device: F.grid_sample (bilinear, align_corners, border) on
             the (1,12,L,Gy,Gx) volume, its forward for the slice, forward and autograd backward for the two backward legs
             (torch cannot run the backward without the forward: its time holds both), and diff / mean / autograd for the total
             variation.  Every call of a leg takes the next of enough buffer sets to hold more than --footprint-mb, so that the
             images come from HBM and not from the 256 MB Infinity Cache; each call's image bytes stand beside the time they
             would take at the 6.3 TB/s a float4 copy reaches on this part (hbm_floor_ms).  A window holds the host's share of a
             call too; with --rocprof the kernels' own time (device_us) is taken from a rocprofv3 kernel trace of a child
             process that makes the same calls.
  iteration  a whole training iteration at --workload (tools/bench_trainer_step.py's fused_in_place leg) with a grid table --
             slice in front of the loss, its backward behind it, tv, the grid's Adam step -- beside none.
Each comparison alternates its legs in one process (harness.alternate: every leg warmed, then `repeats` rounds of one timed
window per leg, a window being `--steps` calls between two device events).  No ratio is asserted.

    python tools/bench_bilateral.py [--out profiles/bilateral_bench.json] [--sizes 1920x1088,976x544] [--grid 16x16x8] [--steps N]
                                    [--warmup N] [--repeats N] [--workload cfg3_headline] [--skip-iteration] [--rocprof] [--quick]
--quick: a rehearsal at sizes where every number is an overhead (96x64 and 52x36, two buffer sets, 2 + 1 calls, 2 rounds, the
20 000-row workload, no kernel trace).
"""
import argparse
import os

import harness as H
import torch
import torch.nn.functional as F

from taichi_3d_gaussian_splatting_amd import bilateral

DEV = "cuda:0"
SIZES = "1920x1088,976x544"
HBM_BYTES_PER_S = 6.3e12            # achievable: a float4 copy
KEYS = ("component", "method", "grid", "calls_ms", "training_iteration_ms", "notes")
KERNELS = {"slice": ("k_bilateral_slice",), "backward": ("k_bilateral_gather", "k_bilateral_backward_image"),
           "backward_image_only": ("k_bilateral_backward_image",), "tv": ("k_bilateral_tv",)}


class Ring:
    """n sets of tensors made by make(i); next() walks them"""

    def __init__(self, make, n):
        self.sets, self.i = [make(i) for i in range(n)], -1

    def next(self):
        self.i = (self.i + 1) % len(self.sets)
        return self.sets[self.i]


def torch_slice(x_3hw, grid):
    """the header's mathematics through grid_sample; x (3,H,W) of any strides, grid (Gy,Gx,L,12)"""
    _, Hh, W = x_3hw.shape
    kw = dict(dtype=x_3hw.dtype, device=x_3hw.device)
    xn = torch.linspace(-1, 1, W, **kw) if W > 1 else torch.full((1,), -1.0, **kw)
    yn = torch.linspace(-1, 1, Hh, **kw) if Hh > 1 else torch.full((1,), -1.0, **kw)
    c = bilateral.LUMINANCE
    zn = 2.0 * (c[0] * x_3hw[0] + c[1] * x_3hw[1] + c[2] * x_3hw[2]).clamp(0.0, 1.0) - 1.0
    coords = torch.stack([xn[None, :].expand(Hh, W), yn[:, None].expand(Hh, W), zn], dim=-1)[None, None]
    M = F.grid_sample(grid.permute(3, 2, 0, 1)[None], coords, mode="bilinear", align_corners=True, padding_mode="border")[0, :, 0]
    M = M.reshape(3, 4, Hh, W)
    return (M[:, :3] * x_3hw[None]).sum(1) + M[:, 3]


def torch_tv(grid):
    return sum((torch.diff(grid, dim=a) ** 2).mean() for a in (1, 0, 2))


def call_legs(Hh, W, grid, gen, footprint_mb):
    """yields (name, the library's call, the torch restatement, its name, image bytes the kernels have to move) of the calls,
    each over a ring of buffer sets that is freed before the next is made"""
    image_bytes = 3 * Hh * W * 4

    def sets(images):
        return max(2, -(-footprint_mb * 10 ** 6 // (images * image_bytes)))

    def image(i):
        return torch.rand(Hh, W, 3, device=DEV, generator=gen)

    ring = Ring(lambda i: (image(i), torch.empty(Hh, W, 3, device=DEV)), sets(2))

    def hip_slice():
        x, c = ring.next()
        bilateral.slice_forward(x.permute(2, 0, 1), grid, out=c.permute(2, 0, 1))

    def tch_slice():
        with torch.no_grad():
            torch_slice(ring.next()[0].permute(2, 0, 1), grid)
    yield "slice", hip_slice, tch_slice, "torch_grid_sample", 2 * image_bytes
    del ring
    torch.cuda.empty_cache()

    grad_grid = torch.empty_like(grid)
    ring = Ring(lambda i: (image(i), image(i) - 0.5, torch.empty(Hh, W, 3, device=DEV)), sets(3))

    def hip_backward(both):
        def call():
            x, g, gi = ring.next()
            bilateral.slice_backward(x.permute(2, 0, 1), g.permute(2, 0, 1), grid, grad_image=gi.permute(2, 0, 1),
                                     grad_grid=grad_grid if both else None)
        return call

    def tch_backward(both):
        def call():
            x, g, _ = ring.next()
            xi, gr = x.permute(2, 0, 1).detach().requires_grad_(True), grid.detach().requires_grad_(both)
            torch.autograd.grad(torch_slice(xi, gr), [xi, gr] if both else [xi], g.permute(2, 0, 1))
        return call
    # the gather reads image and upstream again for every vertex of a cell, from L2: its HBM bytes are still the three images
    yield "backward", hip_backward(True), tch_backward(True), "torch_forward_and_autograd", 3 * image_bytes
    yield "backward_image_only", hip_backward(False), tch_backward(False), "torch_forward_and_autograd", 3 * image_bytes
    del ring
    torch.cuda.empty_cache()

    value = torch.empty(1, device=DEV)

    def hip_tv():
        bilateral.tv(grid, weight=10.0, grad_grid=grad_grid, value=value)

    def tch_tv():
        gr = grid.detach().requires_grad_(True)
        grad_grid.add_(torch.autograd.grad(torch_tv(gr), gr)[0], alpha=10.0)
    yield "tv", hip_tv, tch_tv, "torch_autograd", 3 * grid.numel() * 4


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--sizes", default=SIZES, help="WxH of the images, comma separated")
    ap.add_argument("--grid", default="16x16x8", help="GxxGyxL of the grid")
    ap.add_argument("--steps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=20, help="untimed calls of every leg")
    ap.add_argument("--repeats", type=int, default=5, help="alternating rounds")
    ap.add_argument("--footprint-mb", type=int, default=600, help="bytes the buffer sets of a leg hold together, at least")
    ap.add_argument("--workload", default="cfg3_headline")
    ap.add_argument("--skip-iteration", action="store_true")
    ap.add_argument("--rocprof", action="store_true", help="the kernels' own time by a rocprofv3 kernel trace of a child process")
    ap.add_argument("--quick", action="store_true", help="a rehearsal at tiny sizes: every number is an overhead")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.quick:
        a.sizes, a.workload, a.footprint_mb, a.steps, a.warmup, a.repeats, a.rocprof = "96x64,52x36", "tiny_rehearsal", 0, 2, 1, 2, False
    H.require_gpu("bench_bilateral.py")
    Gx, Gy, L = (int(v) for v in a.grid.lower().split("x"))
    bilateral.check_shape(Gx, Gy, L)
    out = {"component": "bilateral grids: slice, backward, total variation and training iteration, 1x MI355X",
           "method": f"harness.alternate: {a.warmup} warm calls per leg, {a.repeats} rounds of one {a.steps}-call window per leg between device "
                     f"events; every call on the next of enough buffer sets to hold {a.footprint_mb} MB",
           "grid": {"grid_x": Gx, "grid_y": Gy, "grid_l": L, "bytes": Gx * Gy * L * 48}, "calls_ms": {}, "notes": []}
    gen = torch.Generator(device=DEV).manual_seed(0)
    identity = torch.tensor(bilateral.IDENTITY, device=DEV).repeat(Gy, Gx, L, 1)
    grid = (identity + 0.05 * torch.randn(identity.shape, device=DEV, generator=gen)).contiguous()
    if a.child:                 # rocprofv3 target: the calls at the first size, warm-up included in the averages' calls
        W, Hh = (int(v) for v in a.sizes.split(",")[0].lower().split("x"))
        for _, hip, _, _, _ in call_legs(Hh, W, grid, gen, a.footprint_mb):
            for _ in range(a.warmup + a.steps):
                hip()
            torch.cuda.synchronize()
        return
    for size in a.sizes.split(","):
        W, Hh = (int(v) for v in size.lower().split("x"))
        rec = {"height": Hh, "width": W, "image_mb": round(3 * Hh * W * 4 / 1e6, 3)}
        for name, hip, tch, other, nbytes in call_legs(Hh, W, grid, gen, a.footprint_mb):
            leg = H.alternate({"hip": hip, other: tch}, a.steps, a.warmup, a.repeats)
            leg["bytes"] = nbytes
            leg["hbm_floor_ms"] = round(nbytes / HBM_BYTES_PER_S * 1e3, 5)
            leg["torch_over_hip"] = round(leg[other]["median_ms"] / leg["hip"]["median_ms"], 3)
            rec[name] = leg
        if a.rocprof:
            # the windows above hold the host's share of a call too: the kernels' own time comes from a kernel trace of a child
            # process that makes the same calls.  The image pass of the backward runs in both backward legs: its average is over both.
            rows = H.rocprof_kernel_stats([os.path.abspath(__file__), "--sizes", size, "--grid", a.grid, "--steps", str(a.steps * a.repeats),
                                           "--warmup", str(a.warmup), "--footprint-mb", str(a.footprint_mb), "--child"], ("k_bilateral_",), seconds=240)
            rec["kernels_rocprofv3"] = rows
            for name, parts in KERNELS.items():
                value = round(sum(r["avg_us"] for k, r in rows.items() if any(part in k for part in parts)), 3)
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
        table = bilateral.BilateralGridTable(8, DEV, bilateral.BilateralGridConfig(grid_x=Gx, grid_y=Gy, grid_l=L, num_iterations=30_000))
        loss_fn = LossFunction(LossFunction.LossFunctionConfig())
        gt = torch.rand(3, s.height, s.width, device=DEV, generator=gen)
        count = [0]

        def iteration(mode):
            def it():
                count[0] += 1
                view = count[0] % table.num_views
                of.zero_grad(); op.zero_grad()
                img = rast(inp)[0].permute(2, 0, 1)
                if mode == "grid":
                    img = bilateral.slice(img, table.row(view))
                loss_fn(img, gt, point_invalid_mask=inp.point_invalid_mask, pointcloud_features=inp.point_cloud_features,
                        clamp_predicted=True)[0].backward()
                if mode == "grid":
                    bilateral.tv(table.grids[view], weight=table.config.tv_weight, grad_grid=table.grad, value=table.tv_value)
                of.step(); op.step()
                if mode == "grid":
                    table.step(view, count[0])
                controller.refinement()
            return it
        rec = H.alternate({"grid": iteration("grid"), "none": iteration("none")}, a.steps, a.warmup, a.repeats)
        rec["grid_minus_none_ms"] = round(rec["grid"]["median_ms"] - rec["none"]["median_ms"], 5)
        rec["grid_over_none"] = round(rec["grid"]["median_ms"] / rec["none"]["median_ms"], 4)
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
