#!/usr/bin/env python3
"""Measure depth supervision (include/gs_depth.h, depth.py), on cuda:0:
  loss       at every --sizes image, with half the target valid: gs_depth_loss_forward and gs_depth_loss_backward as the trainer
             calls them -- "metric" (inverse depth, L1, no fit: 2 launches forward) and "relative" (the closed-form scale and
             shift: 4 launches forward) -- beside the same formulas in torch operations on the same device.
  resample   gs_depth_resample of a uint16 map of the first size at factors 1, 2 and 4, beside a torch restatement:
             F.interpolate(antialias=True) of v z and of v, then the division and the coverage test.
             Every call of a leg takes the next of enough buffer sets to hold more than --footprint-mb, so that the planes come
             from HBM and not from the 256 MB Infinity Cache; each call's bytes stand beside the time they would take at the
             6.3 TB/s a float4 copy reaches on this part (hbm_floor_ms).  A window holds the host's share of a call too; with
             --rocprof the kernels' own time (kernels_rocprofv3, with its ratio to the floor) is taken from a rocprofv3 kernel trace of a child process that makes the
             same calls, in a run of its own.
  iteration  a whole training iteration at --workload with the depth term ("metric": the rasteriser's depth backward, one
             resample, the loss forward and backward) beside "none".
  margins    with --margins-out: the two seeded 120-iteration runs of tests/test_gpu_trainer_depth.py, with depth="metric" and
             without -- the validation depth error and PSNR of both, written to that file (profiles/depth_margins.json).
Each comparison alternates its legs in one process (harness.alternate).  No ratio is asserted.

    python tools/bench_depth_loss.py [--out profiles/depth_loss_bench.json] [--sizes 1920x1088,976x544] [--steps N] [--warmup N]
                                     [--repeats N] [--workload cfg3_headline] [--skip-iteration] [--rocprof]
                                     [--margins-out profiles/depth_margins.json]
"""
import argparse
import os
import sys
import tempfile

import harness as H
import torch
import torch.nn.functional as F

from taichi_3d_gaussian_splatting_amd import depth

DEV = "cuda:0"
SIZES = "1920x1088,976x544"
FACTORS = (1, 2, 4)
HBM_BYTES_PER_S = 6.3e12            # achievable: a float4 copy
KEYS = ("component", "method", "launches", "loss_ms", "resample_ms", "training_iteration_ms", "notes")
MODES = {"metric": depth.loss_flags("inverse", "l1"), "relative": depth.loss_flags("inverse", "l1", align=True, target_is_inverse=True)}


class Ring:
    """n sets of tensors made by make(i); next() walks them"""

    def __init__(self, make, n):
        self.sets, self.i = [make(i) for i in range(n)], -1

    def next(self):
        self.i = (self.i + 1) % len(self.sets)
        return self.sets[self.i]


def torch_loss(D, Z, w_t, flags, backward):
    """the header's formulas in torch operations, float32 planes and float64 sums; -> (loss, grad or None)"""
    zero = torch.zeros((), device=D.device)
    w = torch.where(w_t > 0, w_t, zero)
    selected = (w > 0) & torch.isfinite(Z) & (Z > 0) & torch.isfinite(D) & (D > 0)
    w = torch.where(selected, w, zero)
    x = torch.where(selected, 1.0 / D if flags & depth.INVERT_PREDICTED else D, zero)
    y = torch.where(selected, 1.0 / Z if flags & depth.INVERT_TARGET else Z, zero)
    S_w = w.sum(dtype=torch.float64)
    if flags & depth.ALIGN:
        wy = w * y
        S_y, S_x, S_yy, S_xy = (v.sum(dtype=torch.float64) for v in (wy, w * x, wy * y, wy * x))
        det = S_w * S_yy - S_y * S_y
        s = torch.where(det > 1e-12 * S_w * S_yy, (S_w * S_xy - S_y * S_x) / det, torch.zeros_like(det))
        t = (S_x - s * S_y) / S_w
        s, t = s.float(), t.float()
    else:
        s, t = 1.0, 0.0
    r = torch.where(selected, x - (s * y + t), zero)
    rho = r * r if flags & depth.L2 else r.abs()
    loss = ((w * rho).sum(dtype=torch.float64) / S_w).float()
    if not backward:
        return loss, None
    grad = w * (2.0 * r if flags & depth.L2 else torch.sign(r)) / S_w.float()
    if flags & depth.INVERT_PREDICTED:
        grad = grad * -(x * x)
    return loss, grad


def torch_resample(src_u16_as_f32, valid, size_full, crop, min_coverage):
    """the restatement: the antialiased resize of v z and of v, the division where the coverage allows it"""
    both = torch.stack([src_u16_as_f32 * valid, valid])[None]
    if tuple(size_full) != tuple(both.shape[-2:]):
        both = F.interpolate(both, size=size_full, mode="bilinear", antialias=True, align_corners=False)
    num, den = both[0, 0, :crop[0], :crop[1]], both[0, 1, :crop[0], :crop[1]]
    ok = (den > 0) & (den >= min_coverage)
    return torch.where(ok, num / torch.where(ok, den, torch.ones_like(den)), torch.zeros_like(num)), torch.where(ok, den, torch.zeros_like(den))


def sets_for(footprint_mb, set_bytes):
    return max(2, -(-footprint_mb * 10 ** 6 // max(set_bytes, 1)))


def loss_legs(Hh, W, gen, footprint_mb):
    """yields (mode, call, the library's leg, the torch leg, bytes the kernels must move)"""
    plane = Hh * W * 4

    def make(i):
        Z = 1.0 + 8.0 * torch.rand(Hh, W, device=DEV, generator=gen)
        D = Z * (0.9 + 0.2 * torch.rand(Hh, W, device=DEV, generator=gen))
        w_t = (torch.rand(Hh, W, device=DEV, generator=gen) < 0.5).float()          # half the target valid
        return D, Z, w_t, torch.empty(Hh, W, device=DEV), torch.empty(depth.LOSS_TERMS, device=DEV)

    ring = Ring(make, sets_for(footprint_mb, 4 * plane))
    for mode, flags in MODES.items():
        passes = 2 if flags & depth.ALIGN else 1

        def hip_forward(flags=flags):
            D, Z, w_t, _, terms = ring.next()
            depth.depth_loss_forward(D, Z, w_t, None, flags, terms=terms)

        def hip_backward(flags=flags):
            D, Z, w_t, g, terms = ring.next()
            depth.depth_loss_backward(D, Z, w_t, None, flags, terms, out=g)
        for s in ring.sets:                 # the backward reads terms the forward wrote
            depth.depth_loss_forward(s[0], s[1], s[2], None, flags, terms=s[4])
        yield mode, "forward", hip_forward, lambda flags=flags: torch_loss(*ring.next()[:3], flags, False), passes * 3 * plane
        yield mode, "backward", hip_backward, lambda flags=flags: torch_loss(*ring.next()[:3], flags, True), 4 * plane
    del ring
    torch.cuda.empty_cache()


def resample_legs(Hh, W, gen, footprint_mb):
    """yields (factor, the library's leg, the torch leg, bytes) on a uint16 (Hh,W) map with a tenth of its samples holes"""
    from taichi_3d_gaussian_splatting_amd.targets import downsampled_geometry
    for factor in FACTORS:
        h_full, w_full, h, w = downsampled_geometry(Hh, W, factor)

        def make(i):
            raw = torch.randint(500, 60000, (Hh, W), device=DEV, generator=gen, dtype=torch.int32)
            raw = torch.where(torch.rand(Hh, W, device=DEV, generator=gen) < 0.1, torch.zeros_like(raw), raw)
            u16 = raw.to(torch.int16).view(torch.uint16)
            as_f32 = raw.float() * 0.001
            return u16, as_f32, (raw != 0).float(), torch.empty(2, h, w, device=DEV)

        ring = Ring(make, sets_for(footprint_mb, Hh * W * 2 + 8 * h * w))

        def hip():
            u16, _, _, out = ring.next()
            depth.depth_resample(u16, (h_full, w_full), (h, w), depth_scale=0.001, min_coverage=0.5, out=out)

        def tch():
            _, z, v, _ = ring.next()
            torch_resample(z, v, (h_full, w_full), (h, w), 0.5)
        yield factor, (h, w), hip, tch, Hh * W * 2 + 8 * h * w
        del ring
        torch.cuda.empty_cache()


def margins(path):
    sys.path.insert(0, os.path.join(H.ROOT, "tests"))
    import depth_trainer_util as DU
    import trainer_util as TU
    with tempfile.TemporaryDirectory(prefix="depth_margins_") as root:
        base = TU.write_dataset(os.path.join(root, "data"), DEV, initial=TU.perturbed(TU.ground_truth_scene()))
        data = DU.add_depth(base, os.path.join(root, "data"), DEV)
        runs = DU.supervised_and_plain_runs(data, os.path.join(root, "runs"), DEV)
    doc = {"run": "trainer_util.SMOKE from the perturbed scene, seed 0, depth weight " + str(DU.SHORT_RUN),
           "validation_depth_error": {k: round(v["depth_error"], 6) for k, v in runs.items()},
           "validation_psnr": {k: round(v["psnr"], 4) for k, v in runs.items()},
           "validation_depth_loss_metric": round(float(runs["metric"]["means"]["depth_loss"]), 8)}
    H.write_json(doc, path)


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
    ap.add_argument("--margins-out", help="also make the two training runs and write their depth errors and PSNRs here")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    H.require_gpu("bench_depth_loss.py")
    out = {"component": "depth supervision: loss forward and backward, target resample and training iteration, 1x MI355X",
           "method": f"harness.alternate: {a.warmup} warm calls per leg, {a.repeats} rounds of one {a.steps}-call window per leg between device "
                     f"events; every call on the next of enough buffer sets to hold {a.footprint_mb} MB",
           "launches": {"forward": depth.FORWARD_LAUNCHES, "forward_align": depth.FORWARD_LAUNCHES_ALIGN, "backward": depth.BACKWARD_LAUNCHES,
                        "resample": 1},
           "loss_ms": {}, "resample_ms": {}, "notes": []}
    gen = torch.Generator(device=DEV).manual_seed(0)
    sizes = [tuple(int(v) for v in s.lower().split("x")) for s in a.sizes.split(",")]
    if a.child:                 # rocprofv3 target: every library leg at the first size
        W, Hh = sizes[0]
        for _, _, hip, _, _ in loss_legs(Hh, W, gen, a.footprint_mb):
            for _ in range(a.warmup + a.steps):
                hip()
            torch.cuda.synchronize()
        for _, _, hip, _, _ in resample_legs(Hh, W, gen, a.footprint_mb):
            for _ in range(a.warmup + a.steps):
                hip()
            torch.cuda.synchronize()
        return
    for W, Hh in sizes:
        rec = {"height": Hh, "width": W, "plane_mb": round(Hh * W * 4 / 1e6, 3)}
        for mode, call, hip, tch, nbytes in loss_legs(Hh, W, gen, a.footprint_mb):
            leg = H.alternate({"hip": hip, "torch": tch}, a.steps, a.warmup, a.repeats)
            leg["bytes"] = nbytes
            leg["hbm_floor_ms"] = round(nbytes / HBM_BYTES_PER_S * 1e3, 5)
            leg["torch_over_hip"] = round(leg["torch"]["median_ms"] / leg["hip"]["median_ms"], 3)
            rec.setdefault(mode, {})[call] = leg
        out["loss_ms"][f"{W}x{Hh}"] = rec
    W, Hh = sizes[0]
    for factor, (h, w), hip, tch, nbytes in resample_legs(Hh, W, gen, a.footprint_mb):
        leg = H.alternate({"hip": hip, "torch": tch}, a.steps, a.warmup, a.repeats)
        leg.update(source=f"{W}x{Hh}", height=h, width=w, bytes=nbytes, hbm_floor_ms=round(nbytes / HBM_BYTES_PER_S * 1e3, 5))
        leg["torch_over_hip"] = round(leg["torch"]["median_ms"] / leg["hip"]["median_ms"], 3)
        out["resample_ms"][f"factor_{factor}"] = leg
    if a.rocprof:
        # the windows above hold the host's share of a call too: the kernels' own time comes from a kernel trace of a child
        # process that makes the same calls at the first size.  (Both loss modes launch k_depth_residual and k_depth_loss_backward,
        # and the three factors one k_depth_resample: a row is the mean over them.)
        rows = H.rocprof_kernel_stats([os.path.abspath(__file__), "--sizes", f"{W}x{Hh}", "--steps", str(a.steps * a.repeats), "--warmup",
                                       str(a.warmup), "--footprint-mb", str(a.footprint_mb), "--child"], ("k_depth_",), seconds=300)
        plane = Hh * W * 4
        floors_us = {"k_depth_moments": 3 * plane, "k_depth_residual": 3 * plane, "k_depth_loss_backward": 4 * plane}
        for name, row in rows.items():
            for kernel, nbytes in floors_us.items():
                if kernel in name:
                    row["bytes"] = nbytes
                    row["device_over_hbm_floor"] = round(row["avg_us"] / (nbytes / HBM_BYTES_PER_S * 1e6), 3)
        out["loss_ms"][f"{W}x{Hh}"]["kernels_rocprofv3"] = rows
    else:
        out["loss_ms"][f"{W}x{Hh}"]["kernels_rocprofv3"] = "not measured"

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
        rast = {}
        for mode in ("metric", "none"):
            cfg = Rast.GaussianPointCloudRasterisationConfig()
            cfg.differentiable_depth = mode == "metric"
            rast[mode] = Rast(cfg, backward_valid_point_hook=controller.update)
        of, op = FusedAdam([inp.point_cloud_features], lr=1e-3), FusedAdam([inp.point_cloud], lr=1e-5)
        loss_fn = LossFunction(LossFunction.LossFunctionConfig())
        gt = torch.rand(3, s.height, s.width, device=DEV, generator=gen)
        with torch.no_grad():
            rendered = rast["none"](inp)[1]
        source = (rendered * 1.05 / 0.001).clamp(0, 65535).to(torch.int32)
        source = torch.where(torch.rand(s.height, s.width, device=DEV, generator=gen) < 0.5, source, torch.zeros_like(source))
        source = source.to(torch.int16).view(torch.uint16)
        target = torch.empty(2, s.height, s.width, device=DEV)

        def iteration(mode):
            def it():
                of.zero_grad(); op.zero_grad()
                image, image_depth, _ = rast[mode](inp)
                loss = loss_fn(image.permute(2, 0, 1), gt, point_invalid_mask=inp.point_invalid_mask, pointcloud_features=inp.point_cloud_features,
                               clamp_predicted=True)[0]
                if mode == "metric":
                    depth.depth_resample(source, (s.height, s.width), depth_scale=0.001, out=target)
                    loss = loss + 0.5 * depth.depth_loss_flags(image_depth, target[0], target[1], None, MODES["metric"])
                loss.backward()
                of.step(); op.step()
                controller.refinement()
            return it
        rec = H.alternate({"metric": iteration("metric"), "none": iteration("none")}, a.steps, a.warmup, a.repeats)
        rec["metric_minus_none_ms"] = round(rec["metric"]["median_ms"] - rec["none"]["median_ms"], 5)
        rec["metric_over_none"] = round(rec["metric"]["median_ms"] / rec["none"]["median_ms"], 4)
        rec["workload"], rec["height"], rec["width"] = a.workload, s.height, s.width
        out["training_iteration_ms"] = rec
        grad_bench = os.path.join(H.ROOT, "profiles", "depth_grad_bench.json")
        if a.workload == "cfg3_headline" and os.path.exists(grad_bench):
            import json
            modes = json.load(open(grad_bench))["modes"]
            share = modes["image+depth"]["ms_median"] - modes["image"]["ms_median"]
            out["notes"].append(f"training_iteration_ms: of the {rec['metric_minus_none_ms']} ms the depth term adds, the rasteriser's depth backward "
                                f"is {share:.3f} ms (profiles/depth_grad_bench.json: image+depth {modes['image+depth']['ms_median']:.3f} ms against "
                                f"image {modes['image']['ms_median']:.3f} ms)")

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
    if a.margins_out:
        margins(a.margins_out)


if __name__ == "__main__":
    main()
