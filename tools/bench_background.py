#!/usr/bin/env python3
"""Measure the background behind the splats (include/gs_background.h, background.py), on cuda:0:
  calls      at every --sizes image and for bands 0 (a solid colour) and 3 (the full sky): gs_background_composite and
             gs_background_backward (both gradients) on the rasteriser's interleaved layout, beside the same formulas written
             in torch operations on the same device (the direction, the basis and the colour of every pixel, then the
             composite; the backward as the selection, a product-sum for grad_alpha and one matmul for grad_coef).  Every call
             of a leg takes the next of enough buffer sets to hold more than --footprint-mb, so that the images come from HBM
             and not from the 256 MB Infinity Cache; each call's bytes (28 per pixel forward, 20 backward) stand beside the time
             they would take at the 6.3 TB/s a float4 copy reaches on this part (hbm_floor_ms).  A window holds the host's share
             of a call too; with --rocprof the kernels' own time (device_us: the image pass and, for the backward, its finishing
             kernel) is taken from a rocprofv3 kernel trace of a child process that makes the same calls.
  iteration  a whole training iteration at --workload (tools/bench_trainer_step.py's fused_in_place leg) with background
             "sky" -- the forward's accumulated alpha, the composite in front of the loss, its backward behind it, the alpha
             gradient through the rasteriser's backward, the sky's Adam step -- beside "none".
Each comparison alternates its legs in one process (harness.alternate: every leg warmed, then `repeats` rounds of one timed
window per leg, a window being `--steps` calls between two device events).  No ratio is asserted.

    python tools/bench_background.py [--out profiles/background_bench.json] [--sizes 1920x1088,976x544] [--bands 0,3] [--steps N]
                                     [--warmup N] [--repeats N] [--workload cfg3_headline] [--skip-iteration] [--rocprof]
"""
import argparse
import os

import harness as H
import torch

from taichi_3d_gaussian_splatting_amd import background

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


def torch_colours(coef, bands, q, K, Hh, W):
    """-> (c (H,W,3), Y (H,W,Kn)): the header's formulas in torch operations (tests/background_ref.py's, on tensors)"""
    import background_ref as ref
    Kn = (bands + 1) ** 2
    if bands == 0:
        Y = [torch.ones(Hh, W, device=DEV)]
    else:
        py, px = torch.meshgrid(torch.arange(Hh, device=DEV, dtype=torch.float32), torch.arange(W, device=DEV, dtype=torch.float32), indexing="ij")
        Y = ref.basis(px, py, q.reshape(4), K.reshape(9), c=float, sqrt=torch.sqrt)[:Kn]
        Y[0] = torch.ones_like(px)
    c = ref.colour(coef, Y + [None] * (16 - Kn), bands)
    return torch.stack([ci.expand(Hh, W) if ci.dim() == 0 else ci for ci in c], dim=2), torch.stack(Y, dim=2)


def torch_composite(x_hw3, A, coef, bands, q, K):
    c, _ = torch_colours(coef, bands, q, K, *A.shape)
    return x_hw3 + (1.0 - A)[:, :, None] * c


def torch_backward(g_hw3, A, coef, bands, q, K):
    c, Y = torch_colours(coef, bands, q, K, *A.shape)
    selected = (g_hw3 != 0).any(dim=2)
    grad_alpha = torch.where(selected, -(g_hw3 * c).sum(dim=2), torch.zeros_like(A))
    gt = torch.where(selected[:, :, None], g_hw3 * (1.0 - A)[:, :, None], torch.zeros_like(g_hw3))
    return grad_alpha, gt.reshape(-1, 3).t() @ Y.reshape(-1, Y.shape[2])


def call_legs(Hh, W, bands, coef, q, K, gen, footprint_mb):
    """yields (name, the library's call, the torch restatement, bytes the kernel has to move) of the two calls, each over a
    ring of buffer sets that is freed before the next is made"""
    pixels = Hh * W

    def sets(bytes_per_set):
        return max(2, -(-footprint_mb * 10 ** 6 // bytes_per_set))

    def image(i):
        return torch.rand(Hh, W, 3, device=DEV, generator=gen)

    def plane(i):
        return torch.rand(Hh, W, device=DEV, generator=gen)

    ring = Ring(lambda i: (image(i), plane(i), torch.empty(Hh, W, 3, device=DEV)), sets(28 * pixels))

    def hip_composite():
        x, A, out = ring.next()
        background.composite_forward(x.permute(2, 0, 1), A, coef, bands, q, K, out=out.permute(2, 0, 1))
    yield "composite", hip_composite, lambda: torch_composite(*ring.next()[:2], coef, bands, q, K), 28 * pixels
    del ring
    torch.cuda.empty_cache()

    grad_coef = torch.empty(background.COEF_FLOATS, device=DEV)
    ring = Ring(lambda i: (image(i) - 0.5, plane(i), torch.empty(Hh, W, device=DEV)), sets(20 * pixels))

    def hip_backward():
        g, A, ga = ring.next()
        background.composite_backward(g.permute(2, 0, 1), A, coef, bands, q, K, grad_alpha=ga, grad_coef=grad_coef)
    yield "backward", hip_backward, lambda: torch_backward(*ring.next()[:2], coef, bands, q, K), 20 * pixels
    del ring
    torch.cuda.empty_cache()


def camera(Hh, W):
    return torch.tensor([[0.6 * W, 0.0, 0.5 * W], [0.0, 0.6 * W, 0.5 * Hh], [0.0, 0.0, 1.0]], device=DEV)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--sizes", default=SIZES, help="WxH of the images, comma separated")
    ap.add_argument("--bands", default="0,3", help="bands of the background, comma separated")
    ap.add_argument("--steps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=20, help="untimed calls of every leg")
    ap.add_argument("--repeats", type=int, default=5, help="alternating rounds")
    ap.add_argument("--footprint-mb", type=int, default=600, help="bytes the buffer sets of a leg hold together, at least")
    ap.add_argument("--workload", default="cfg3_headline")
    ap.add_argument("--skip-iteration", action="store_true")
    ap.add_argument("--rocprof", action="store_true", help="the kernels' own time by a rocprofv3 kernel trace of a child process")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    H.require_gpu("bench_background.py")
    out = {"component": "background behind the splats: composite, backward and training iteration, 1x MI355X",
           "method": f"harness.alternate: {a.warmup} warm calls per leg, {a.repeats} rounds of one {a.steps}-call window per leg between device "
                     f"events; every call on the next of enough buffer sets to hold {a.footprint_mb} MB",
           "calls_ms": {}, "notes": []}
    gen = torch.Generator(device=DEV).manual_seed(0)
    coef = 0.3 * torch.randn(background.COEF_FLOATS, device=DEV, generator=gen)
    q = torch.tensor([[0.1, 0.3, -0.2, 0.9]], device=DEV)
    all_bands = [int(b) for b in a.bands.split(",")]
    if a.child:                 # rocprofv3 target: the two calls at the first size and the first band count
        W, Hh = (int(v) for v in a.sizes.split(",")[0].lower().split("x"))
        for _, hip, _, _ in call_legs(Hh, W, all_bands[0], coef, q, camera(Hh, W), gen, a.footprint_mb):
            for _ in range(a.warmup + a.steps):
                hip()
            torch.cuda.synchronize()
        return
    for size in a.sizes.split(","):
        W, Hh = (int(v) for v in size.lower().split("x"))
        rec = {"height": Hh, "width": W, "image_mb": round(3 * Hh * W * 4 / 1e6, 3)}
        for bands in all_bands:
            per_band = {}
            for name, hip, tch, nbytes in call_legs(Hh, W, bands, coef, q, camera(Hh, W), gen, a.footprint_mb):
                leg = H.alternate({"hip": hip, "torch": tch}, a.steps, a.warmup, a.repeats)
                leg["bytes"] = nbytes
                leg["hbm_floor_ms"] = round(nbytes / HBM_BYTES_PER_S * 1e3, 5)
                leg["torch_over_hip"] = round(leg["torch"]["median_ms"] / leg["hip"]["median_ms"], 3)
                per_band[name] = leg
            if a.rocprof:
                # the windows above hold the host's share of a call too: the kernels' own time comes from a kernel trace of a
                # child process that makes the same calls
                rows = H.rocprof_kernel_stats([os.path.abspath(__file__), "--sizes", size, "--bands", str(bands), "--steps", str(a.steps * a.repeats),
                                               "--warmup", str(a.warmup), "--footprint-mb", str(a.footprint_mb), "--child"], ("k_background_",),
                                              seconds=240)
                per_band["kernels_rocprofv3"] = rows

                def us(*parts):
                    return round(sum(r["avg_us"] for k, r in rows.items() if any(part in k for part in parts)), 3)
                for name, value in (("composite", us("k_background_composite")), ("backward", us("k_background_backward", "k_background_finish"))):
                    per_band[name]["device_us"] = value
                    per_band[name]["device_over_hbm_floor"] = round(value / (per_band[name]["hbm_floor_ms"] * 1e3), 3)
            else:
                for name in ("composite", "backward"):
                    per_band[name]["device_us"] = "not measured"
            rec[f"bands{bands}"] = per_band
        out["calls_ms"][f"{W}x{Hh}"] = rec

    if a.skip_iteration:
        out["training_iteration_ms"] = "not measured"
    else:
        from taichi_3d_gaussian_splatting_amd import GaussianPointAdaptiveController, GaussianPointCloudRasterisation as Rast
        from taichi_3d_gaussian_splatting_amd.LossFunction import LossFunction
        from taichi_3d_gaussian_splatting_amd.optim import FusedAdam
        from taichi_3d_gaussian_splatting_amd.synthetic import make_scene, scene_input, view_pose
        s = make_scene(a.workload)
        qv, tv = view_pose()
        inp = scene_input(s, qv, tv, DEV, requires_grad=True)
        controller_config = GaussianPointAdaptiveController.GaussianPointAdaptiveControllerConfig()
        controller_config.num_iterations_warm_up = 10 ** 9
        controller = GaussianPointAdaptiveController(
            config=controller_config, maintained_parameters=GaussianPointAdaptiveController.GaussianPointAdaptiveControllerMaintainedParameters(
                pointcloud=inp.point_cloud, pointcloud_features=inp.point_cloud_features, point_invalid_mask=inp.point_invalid_mask,
                point_object_id=inp.point_object_id), seed=0)
        rast = Rast(Rast.GaussianPointCloudRasterisationConfig(), backward_valid_point_hook=controller.update)
        of, op = FusedAdam([inp.point_cloud_features], lr=1e-3), FusedAdam([inp.point_cloud], lr=1e-5)
        model = background.BackgroundModel("sky", DEV, background.BackgroundConfig(colour=(0.5, 0.5, 0.5), bands=2, num_iterations=30_000))
        loss_fn = LossFunction(LossFunction.LossFunctionConfig())
        gt = torch.rand(3, s.height, s.width, device=DEV, generator=gen)
        count = [0]

        def iteration(mode):
            def it():
                count[0] += 1
                of.zero_grad(); op.zero_grad()
                if mode == "sky":
                    img, _, _, alpha = rast(inp, return_accumulated_alpha=True)
                    img = background.composite(img.permute(2, 0, 1), alpha, model.coef_for_step(), model.bands, inp.q_pointcloud_camera.detach(),
                                               inp.camera_info.camera_intrinsics)
                else:
                    img = rast(inp)[0].permute(2, 0, 1)
                loss_fn(img, gt, point_invalid_mask=inp.point_invalid_mask, pointcloud_features=inp.point_cloud_features,
                        clamp_predicted=True)[0].backward()
                of.step(); op.step()
                if mode == "sky":
                    model.step(count[0])
                controller.refinement()
            return it
        rec = H.alternate({"sky": iteration("sky"), "none": iteration("none")}, a.steps, a.warmup, a.repeats)
        rec["sky_minus_none_ms"] = round(rec["sky"]["median_ms"] - rec["none"]["median_ms"], 5)
        rec["sky_over_none"] = round(rec["sky"]["median_ms"] / rec["none"]["median_ms"], 4)
        rec["workload"], rec["height"], rec["width"], rec["bands"] = a.workload, s.height, s.width, model.bands
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
