#!/usr/bin/env python3
"""Measure the geometry regularisers (include/gs_geometry.h, geometry.py), on cuda:0:
  kernels    at every --sizes image: gs_depth_normals, gs_normal_loss_forward / _backward (8-bit style prior in [0, 1], OpenGL frame,
             max_rel_jump 0.1, a pixel weight) and gs_depth_smooth_forward / _backward (inverse depth, first order, the guide and
             a pixel weight) as the trainer calls them, beside the same formulas in torch operations on the same device (float32
             planes, float64 sums; the torch backward leg is the forward and autograd's backward through it).
             Every call of a leg takes the next of enough buffer sets to hold more than --footprint-mb, so that the planes come
             from HBM and not from the 256 MB Infinity Cache; each call's bytes stand beside the time they would take at the
             6.3 TB/s a float4 copy reaches on this part (hbm_floor_ms).  A window holds the host's share of a call too; with
             --rocprof the kernels' own time (kernels_rocprofv3, with its ratio to the floor) is taken from a rocprofv3 kernel
             trace of a child process that makes the same calls, in a run of its own.
  iteration  a whole training iteration at --workload with both terms (the rasteriser's depth backward, both losses forward
             and backward) beside one without.
  margins    with --margins-out: the two seeded 120-iteration runs of tests/test_gpu_trainer_geometry.py, with the terms and
             without -- the validation normal angle and PSNR of both, written to that file (profiles/geometry_margins.json).
Each comparison alternates its legs in one process (harness.alternate).  No ratio is asserted.

    python tools/bench_geometry.py [--out profiles/geometry_bench.json] [--sizes 1920x1088,976x544] [--steps N] [--warmup N]
                                   [--repeats N] [--workload cfg3_headline] [--skip-iteration] [--rocprof]
                                   [--margins-out profiles/geometry_margins.json]
"""
import argparse
import os
import sys
import tempfile

import harness as H
import torch

from taichi_3d_gaussian_splatting_amd import geometry

DEV = "cuda:0"
SIZES = "1920x1088,976x544"
HBM_BYTES_PER_S = 6.3e12            # achievable: a float4 copy
KEYS = ("component", "method", "launches", "tile", "kernels_ms", "training_iteration_ms", "notes")
JUMP, LAMBDA = 0.1, 10.0
NORMAL_FLAGS = geometry.normal_flags(True, "opengl")
SMOOTH_FLAGS = geometry.smooth_flags("inverse", 1)


class Ring:
    """n sets of tensors made by make(i); next() walks them"""

    def __init__(self, make, n):
        self.sets, self.i = [make(i) for i in range(n)], -1

    def next(self):
        self.i = (self.i + 1) % len(self.sets)
        return self.sets[self.i]


def camera(Hh, W):
    return (0.9 * W, 0.9 * W, 0.5 * W, 0.5 * Hh)


def torch_normals(D, K, jump):
    """the header's normal in torch operations on the interior; -> (exists (H-2,W-2), c (3,H-2,W-2), length)"""
    Hh, W = D.shape
    fx, fy, cx, cy = K
    x = torch.arange(1, W - 1, device=D.device, dtype=torch.float32)[None, :]
    y = torch.arange(1, Hh - 1, device=D.device, dtype=torch.float32)[:, None]
    l, r, u, d, m = D[1:-1, :-2], D[1:-1, 2:], D[:-2, 1:-1], D[2:, 1:-1], D[1:-1, 1:-1]
    ok = (l > 0) & (r > 0) & (u > 0) & (d > 0) & (m > 0) & torch.isfinite(l + r + u + d + m)
    dx, dy = r - l, d - u
    if jump > 0:
        ok = ok & (dx.abs() <= jump * m) & (dy.abs() <= jump * m)
    a = lambda k: (x + (k + 0.5 - cx)) / fx         # noqa: E731
    b = lambda k: (y + (k + 0.5 - cy)) / fy         # noqa: E731
    px = torch.stack([a(1) * r - a(-1) * l, b(0) * dx, dx])
    py = torch.stack([a(0) * dy, b(1) * d - b(-1) * u, dy])
    c = torch.linalg.cross(py, px, dim=0)
    q = (c * c).sum(0)
    ok = ok & (q > 0) & torch.isfinite(q)
    return ok, c, torch.where(ok, q, torch.ones_like(q)).sqrt()


def torch_depth_normals(D, K, jump):
    ok, c, length = torch_normals(D, K, jump)
    out = torch.zeros((3,) + tuple(D.shape), device=D.device)
    out[:, 1:-1, 1:-1] = torch.where(ok, c / length, torch.zeros_like(c))
    return out


def torch_normal_loss(D, N, w_n, w_p, K, jump, backward):
    if backward:
        D = D.detach().requires_grad_(True)
    ok, c, length = torch_normals(D, K, jump)
    m = (2.0 * N[:, 1:-1, 1:-1] - 1.0) * torch.tensor([1.0, -1.0, -1.0], device=D.device)[:, None, None]
    k = (m * m).sum(0).sqrt()
    w = torch.clamp(w_n[1:-1, 1:-1], min=0) * torch.clamp(w_p[1:-1, 1:-1], min=0)
    sel = ok & (k >= 0.5) & (w > 0)
    cos = ((c / length) * (m / torch.where(sel, k, torch.ones_like(k)))).sum(0)
    zero = torch.zeros_like(cos)
    loss = (torch.where(sel, w * (1.0 - cos), zero).sum(dtype=torch.float64) / torch.where(sel, w, zero).sum(dtype=torch.float64)).float()
    if backward:
        loss.backward()
        return loss, D.grad
    return loss, None


def torch_smoothness(D, I, w_p, lam, backward):
    if backward:
        D = D.detach().requires_grad_(True)
    valid = (D > 0) & torch.isfinite(D)
    x = torch.where(valid, 1.0 / torch.where(valid, D, torch.ones_like(D)), torch.zeros_like(D))
    a = torch.clamp(w_p, min=0)
    num = den = 0.0
    for sl_i, sl_j in (((slice(None), slice(0, -1)), (slice(None), slice(1, None))), ((slice(0, -1), slice(None)), (slice(1, None), slice(None)))):
        w = a[sl_i] * a[sl_j]
        sel = valid[sl_i] & valid[sl_j] & (w > 0)
        e = torch.exp(-lam * (I[(slice(None),) + sl_j] - I[(slice(None),) + sl_i]).abs().mean(0))
        zero = torch.zeros_like(w)
        num = num + torch.where(sel, w * e * (x[sl_j] - x[sl_i]).abs(), zero).sum(dtype=torch.float64)
        den = den + torch.where(sel, w, zero).sum(dtype=torch.float64)
    loss = (num / den).float()
    if backward:
        loss.backward()
        return loss, D.grad
    return loss, None


def sets_for(footprint_mb, set_bytes):
    return max(2, -(-footprint_mb * 10 ** 6 // max(set_bytes, 1)))


def legs_for(Hh, W, gen, footprint_mb):
    """yields (name, the library's leg, the torch leg, bytes the kernels must move)"""
    plane = Hh * W * 4
    K = camera(Hh, W)

    def make(i):
        yy, xx = torch.meshgrid(torch.arange(Hh, device=DEV, dtype=torch.float32), torch.arange(W, device=DEV, dtype=torch.float32), indexing="ij")
        D = 3.0 + 0.3 * torch.sin(xx / 37.0 + i) + 0.2 * torch.cos(yy / 23.0) + 0.002 * torch.rand(Hh, W, device=DEV, generator=gen)
        D = torch.where(torch.rand(Hh, W, device=DEV, generator=gen) < 0.02, torch.zeros_like(D), D)          # holes
        N = torch.randn(3, Hh, W, device=DEV, generator=gen) * 0.2 + torch.tensor([0.0, 0.0, 1.0], device=DEV)[:, None, None]
        N = (N / N.norm(dim=0) + 1.0) / 2.0
        w_n = (torch.rand(Hh, W, device=DEV, generator=gen) < 0.9).float()
        w_p = torch.rand(Hh, W, device=DEV, generator=gen)
        I = torch.rand(3, Hh, W, device=DEV, generator=gen)
        return dict(D=D.contiguous(), N=N.contiguous(), w_n=w_n, w_p=w_p, I=I, g=torch.empty(Hh, W, device=DEV), n=torch.empty(3, Hh, W, device=DEV),
                    tn=torch.empty(geometry.LOSS_TERMS, device=DEV), ts=torch.empty(geometry.LOSS_TERMS, device=DEV))

    ring = Ring(make, sets_for(footprint_mb, 13 * plane))
    for s in ring.sets:                     # the backwards read the terms the forwards wrote
        geometry.normal_loss_forward(s["D"], K, s["N"], s["w_n"], s["w_p"], JUMP, NORMAL_FLAGS, terms=s["tn"])
        geometry.depth_smooth_forward(s["D"], s["I"], s["w_p"], LAMBDA, SMOOTH_FLAGS, terms=s["ts"])

    def normals():
        s = ring.next()
        geometry.depth_normals(s["D"], K, JUMP, out=s["n"])

    def normal_forward():
        s = ring.next()
        geometry.normal_loss_forward(s["D"], K, s["N"], s["w_n"], s["w_p"], JUMP, NORMAL_FLAGS, terms=s["tn"])

    def normal_backward():
        s = ring.next()
        geometry.normal_loss_backward(s["D"], K, s["N"], s["w_n"], s["w_p"], JUMP, NORMAL_FLAGS, s["tn"], out=s["g"])

    def smooth_forward():
        s = ring.next()
        geometry.depth_smooth_forward(s["D"], s["I"], s["w_p"], LAMBDA, SMOOTH_FLAGS, terms=s["ts"])

    def smooth_backward():
        s = ring.next()
        geometry.depth_smooth_backward(s["D"], s["I"], s["w_p"], LAMBDA, SMOOTH_FLAGS, s["ts"], out=s["g"])

    def t(fn, *names, **kw):
        return lambda: fn(*(ring.next()[n] for n in names[:1]), *[ring.sets[ring.i][n] for n in names[1:]], **kw)
    yield "depth_normals", normals, lambda: torch_depth_normals(ring.next()["D"], K, JUMP), 4 * plane
    yield "normal_loss_forward", normal_forward, t(torch_normal_loss, "D", "N", "w_n", "w_p", K=K, jump=JUMP, backward=False), 6 * plane
    yield "normal_loss_backward", normal_backward, t(torch_normal_loss, "D", "N", "w_n", "w_p", K=K, jump=JUMP, backward=True), 7 * plane
    yield "depth_smooth_forward", smooth_forward, t(torch_smoothness, "D", "I", "w_p", lam=LAMBDA, backward=False), 5 * plane
    yield "depth_smooth_backward", smooth_backward, t(torch_smoothness, "D", "I", "w_p", lam=LAMBDA, backward=True), 6 * plane
    del ring
    torch.cuda.empty_cache()


def leg_of_kernel(name):
    """the leg a traced kernel name belongs to, or None (the finishing kernel); a template argument may print as true, 1 or (bool)1"""
    backward = any(v in name for v in ("<true>", "<1>", "<(bool)1>"))
    for kernel, legs in (("k_normal_loss", ("normal_loss_forward", "normal_loss_backward")), ("k_depth_smooth", ("depth_smooth_forward", "depth_smooth_backward"))):
        if kernel in name:
            return legs[1 if backward else 0]
    return "depth_normals" if "k_depth_normals" in name else None


def margins(path):
    sys.path.insert(0, os.path.join(H.ROOT, "tests"))
    import geometry_trainer_util as GU
    import trainer_util as TU
    with tempfile.TemporaryDirectory(prefix="geometry_margins_") as root:
        base = TU.write_dataset(os.path.join(root, "data"), DEV, initial=TU.perturbed(TU.ground_truth_scene()))
        data = GU.add_normals(base, os.path.join(root, "data"), DEV)
        runs = GU.regularised_and_plain_runs(data, os.path.join(root, "runs"), DEV)
    doc = {"run": "trainer_util.SMOKE from the perturbed scene, seed 0, geometry weights " + str(GU.SHORT_RUN),
           "validation_normal_angle_degrees": {k: round(v["angle"], 4) for k, v in runs.items()},
           "validation_psnr": {k: round(v["psnr"], 4) for k, v in runs.items()},
           "validation_losses_geometry": {k: round(float(v), 8) for k, v in runs["geometry"]["means"].items() if k in ("smooth_loss", "normal_loss")}}
    H.write_json(doc, path)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--sizes", default=SIZES, help="WxH of the images, comma separated")
    ap.add_argument("--steps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=20, help="untimed calls of every leg")
    ap.add_argument("--repeats", type=int, default=5, help="alternating rounds")
    ap.add_argument("--footprint-mb", type=int, default=600, help="bytes the buffer sets of a size hold together, at least")
    ap.add_argument("--workload", default="cfg3_headline")
    ap.add_argument("--skip-iteration", action="store_true")
    ap.add_argument("--rocprof", action="store_true", help="the kernels' own time by a rocprofv3 kernel trace of a child process")
    ap.add_argument("--margins-out", help="also make the two training runs and write their normal angles and PSNRs here")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    H.require_gpu("bench_geometry.py")
    out = {"component": "geometry regularisers: depth normals, normal loss and depth smoothness forward and backward, training iteration, 1x MI355X",
           "method": f"harness.alternate: {a.warmup} warm calls per leg, {a.repeats} rounds of one {a.steps}-call window per leg between device "
                     f"events; every call on the next of enough buffer sets to hold {a.footprint_mb} MB",
           "launches": {"forward": geometry.FORWARD_LAUNCHES, "backward": geometry.BACKWARD_LAUNCHES, "depth_normals": 1},
           "tile": {"height": geometry.TILE_H, "width": geometry.TILE_W, "halo": geometry.HALO},
           "kernels_ms": {}, "notes": []}
    gen = torch.Generator(device=DEV).manual_seed(0)
    sizes = [tuple(int(v) for v in s.lower().split("x")) for s in a.sizes.split(",")]
    if a.child:                 # rocprofv3 target: every library leg at every size
        for W, Hh in sizes:
            for _, hip, _, _ in legs_for(Hh, W, gen, a.footprint_mb):
                for _ in range(a.warmup + a.steps):
                    hip()
                torch.cuda.synchronize()
        return
    for W, Hh in sizes:
        rec = {"height": Hh, "width": W, "plane_mb": round(Hh * W * 4 / 1e6, 3)}
        for name, hip, tch, nbytes in legs_for(Hh, W, gen, a.footprint_mb):
            leg = H.alternate({"hip": hip, "torch": tch}, a.steps, a.warmup, a.repeats)
            leg["bytes"] = nbytes
            leg["hbm_floor_ms"] = round(nbytes / HBM_BYTES_PER_S * 1e3, 5)
            leg["torch_over_hip"] = round(leg["torch"]["median_ms"] / leg["hip"]["median_ms"], 3)
            rec[name] = leg
        if a.rocprof:
            # the windows above hold the host's share of a call too: the kernels' own time comes from a kernel trace of a child
            # process that makes the same calls at this size
            rows = H.rocprof_kernel_stats([os.path.abspath(__file__), "--sizes", f"{W}x{Hh}", "--steps", str(a.steps * a.repeats), "--warmup",
                                           str(a.warmup), "--footprint-mb", str(a.footprint_mb), "--child"],
                                          ("k_depth_normals", "k_normal_loss", "k_depth_smooth", "k_geometry_finish"), seconds=300)
            for name, row in rows.items():
                leg = leg_of_kernel(name)
                if leg is not None:
                    row["bytes"] = rec[leg]["bytes"]
                    row["device_over_hbm_floor"] = round(row["avg_us"] / (rec[leg]["bytes"] / HBM_BYTES_PER_S * 1e6), 3)
            rec["kernels_rocprofv3"] = rows
        else:
            rec["kernels_rocprofv3"] = "not measured"
        out["kernels_ms"][f"{W}x{Hh}"] = rec

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
        for mode in ("geometry", "none"):
            cfg = Rast.GaussianPointCloudRasterisationConfig()
            cfg.differentiable_depth = mode == "geometry"
            rast[mode] = Rast(cfg, backward_valid_point_hook=controller.update)
        of, op = FusedAdam([inp.point_cloud_features], lr=1e-3), FusedAdam([inp.point_cloud], lr=1e-5)
        loss_fn = LossFunction(LossFunction.LossFunctionConfig())
        gt = torch.rand(3, s.height, s.width, device=DEV, generator=gen)
        prior = torch.rand(3, s.height, s.width, device=DEV, generator=gen)
        prior_weight = torch.ones(s.height, s.width, device=DEV)
        K = geometry.intrinsics_tuple(torch.as_tensor(s.camera_intrinsics))

        def iteration(mode):
            def it():
                of.zero_grad(); op.zero_grad()
                image, image_depth, _ = rast[mode](inp)
                loss = loss_fn(image.permute(2, 0, 1), gt, point_invalid_mask=inp.point_invalid_mask, pointcloud_features=inp.point_cloud_features,
                               clamp_predicted=True)[0]
                if mode == "geometry":
                    loss = loss + 0.5 * geometry.depth_smoothness_flags(image_depth, gt, None, LAMBDA, SMOOTH_FLAGS) \
                        + 0.1 * geometry.normal_loss_flags(image_depth, K, prior, prior_weight, None, JUMP, NORMAL_FLAGS)
                loss.backward()
                of.step(); op.step()
                controller.refinement()
            return it
        rec = H.alternate({"geometry": iteration("geometry"), "none": iteration("none")}, a.steps, a.warmup, a.repeats)
        rec["geometry_minus_none_ms"] = round(rec["geometry"]["median_ms"] - rec["none"]["median_ms"], 5)
        rec["geometry_over_none"] = round(rec["geometry"]["median_ms"] / rec["none"]["median_ms"], 4)
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
    if a.margins_out:
        margins(a.margins_out)


if __name__ == "__main__":
    main()
