#!/usr/bin/env python3
"""Measure the 3D smoothing filter (include/gs_filter3d.h, filter3d.py), on cuda:0:
  rate       gs_filter3d_rate at every --rate-shapes pair of rows x views (a synthetic cloud inside and around the frusta of a
             ring of cameras), beside the same formulas in torch operations on the same device, sixteen views to a broadcast.
             The pass is arithmetic, not traffic: pairs per second are reported, and no share of a peak is claimed.
  apply      gs_filter3d_apply and gs_filter3d_apply_backward (out of place, as the autograd node calls it) at every --rows
             count, beside the same formulas in float64 torch operations.  Every call takes the next of enough buffer sets to
             hold more than --footprint-mb; each call's bytes (452 and 468 per row) stand beside the time they would take at
             the 6.3 TB/s a float4 copy reaches on this part (hbm_floor_ms).  A window holds the host's share of a call too;
             with --rocprof the kernels' own time (device_us) is taken from a rocprofv3 kernel trace of a child process that
             makes the same calls.
  iteration  a whole training iteration at --workload (tools/bench_trainer_step.py's fused_in_place leg) with the filter's
             apply node in front of the rasteriser, beside the iteration without it.
Each comparison alternates its legs in one process (harness.alternate: every leg warmed, then `repeats` rounds of one timed
window per leg, a window being `--steps` calls between two device events).  No ratio is asserted.

    python tools/bench_filter3d.py [--out profiles/filter3d_bench.json] [--rate-shapes 500000x100,500000x300,2000000x100]
                                   [--rows 500000,2000000] [--steps N] [--warmup N] [--repeats N] [--workload cfg3_headline]
                                   [--skip-iteration] [--rocprof]
"""
import argparse
import os

import harness as H
import torch

from taichi_3d_gaussian_splatting_amd import filter3d

DEV = "cuda:0"
RATE_SHAPES = "500000x100,500000x300,2000000x100"
ROWS = "500000,2000000"
HBM_BYTES_PER_S = 6.3e12            # achievable: a float4 copy
APPLY_BYTES, BACKWARD_BYTES = 224 + 4 + 224, 224 + 16 + 4 + 224       # per row: the rows read, the rate, the rows written
W, HH, NEAR, MARGIN = 1920, 1088, 0.8, 0.15
KEYS = ("component", "method", "rate_ms", "apply_ms", "training_iteration_ms", "notes")


class Ring:
    """n sets of tensors made by make(i); next() walks them"""

    def __init__(self, make, n):
        self.sets, self.i = [make(i) for i in range(n)], -1

    def next(self):
        self.i = (self.i + 1) % len(self.sets)
        return self.sets[self.i]


def ring_views(n_views, gen):
    """n_views cameras on a ring of radius 6 around the origin, looking at it: (V,16)"""
    angle = 2 * torch.pi * torch.arange(n_views, device=DEV, dtype=torch.float64) / max(n_views, 1)
    centre = torch.stack([6.0 * torch.sin(angle), 0.5 * torch.rand(n_views, device=DEV, generator=gen, dtype=torch.float64) - 0.25,
                          -6.0 * torch.cos(angle)], dim=1)
    z = -centre / centre.norm(dim=1, keepdim=True)
    up = torch.tensor([0.0, 1.0, 0.0], device=DEV, dtype=torch.float64).expand_as(z)
    x = torch.linalg.cross(up, z)
    x = x / x.norm(dim=1, keepdim=True)
    y = torch.linalg.cross(z, x)
    R = torch.stack([x, y, z], dim=1)
    t = -(R @ centre[:, :, None])[:, :, 0]
    k = torch.tensor([0.6 * W, 0.62 * W, 0.5 * W, 0.5 * HH], device=DEV, dtype=torch.float64).expand(n_views, 4)
    return torch.cat([R.reshape(n_views, 9), t, k], dim=1).to(torch.float32).contiguous()


def torch_rate(pc, mask, views, chunk=16):
    """the header's formulas in torch operations, `chunk` views to a broadcast"""
    x, y, z = pc[:, 0:1], pc[:, 1:2], pc[:, 2:3]
    best = torch.zeros(pc.shape[0], device=DEV)
    lo_x, hi_x, lo_y, hi_y = -MARGIN * W, (1 + MARGIN) * W, -MARGIN * HH, (1 + MARGIN) * HH
    for v0 in range(0, views.shape[0], chunk):
        w = views[v0:v0 + chunk].t()
        p0 = ((w[0] * x + w[1] * y) + w[2] * z) + w[9]
        p1 = ((w[3] * x + w[4] * y) + w[5] * z) + w[10]
        p2 = ((w[6] * x + w[7] * y) + w[8] * z) + w[11]
        u, v = (w[12] * p0) / p2 + w[14], (w[13] * p1) / p2 + w[15]
        c = torch.maximum(w[12], w[13]) / p2
        sees = (p2 > NEAR) & (lo_x <= u) & (u <= hi_x) & (lo_y <= v) & (v <= hi_y) & (c > 0)
        best = torch.maximum(best, torch.where(sees, c, torch.zeros_like(c)).amax(dim=1))
    valid = mask == 0
    seen = valid & (best > 0)
    smallest = torch.where(seen, best, torch.full_like(best, float("inf"))).min() if best.numel() else best.sum()
    return torch.where(valid, torch.where(seen, best, smallest), torch.full_like(best, float("inf")))


def torch_terms(features, rate, k):
    f = (k / rate).double()
    on = f > 0
    v = (f * f)[:, None]
    s = torch.exp(features[:, 4:7].double()) ** 2
    t = s + v
    r = s / t
    c = torch.sqrt(r[:, 0] * r[:, 1] * r[:, 2])
    E = torch.exp(-features[:, 7].double())
    return on, t, r, c, E, (1.0 - c) + E


def torch_apply(features, rate, k):
    on, t, r, c, E, D = torch_terms(features, rate, k)
    q = features[:, :4] / features[:, :4].norm(dim=1, keepdim=True)
    out = features.clone()
    out[:, :4] = torch.where(on[:, None], q, features[:, :4])
    out[:, 4:7] = torch.where(on[:, None], (0.5 * torch.log(t)).float(), features[:, 4:7])
    out[:, 7] = torch.where(on, (torch.log(c) - torch.log(D)).float(), features[:, 7])
    return out


def torch_backward(grad, features, rate, k):
    on, t, r, c, E, D = torch_terms(features, rate, k)
    ga, gls = grad[:, 7].double(), grad[:, 4:7].double()
    out = grad.clone()
    down = gls * r + (ga * (1.0 + c / D))[:, None] * (1.0 - r)
    out[:, 4:7] = torch.where(on[:, None], down.float(), grad[:, 4:7])
    out[:, 7] = torch.where(on, (ga * E / D).float(), grad[:, 7])
    return out


def cloud(n, gen):
    """(point_cloud, mask): rows inside and around the cameras' ring, a hundredth of them invalid"""
    pc = 8.0 * torch.rand(n, 3, device=DEV, generator=gen) - 4.0
    mask = (torch.rand(n, device=DEV, generator=gen) < 0.01).to(torch.int8)
    return pc, mask


def feature_rows(n, gen):
    feat = torch.randn(n, 56, device=DEV, generator=gen)
    feat[:, 4:7] = -6.0 + 4.0 * torch.rand(n, 3, device=DEV, generator=gen)
    feat[:, 7] = -4.0 + 8.0 * torch.rand(n, device=DEV, generator=gen)
    return feat


def apply_legs(n, k, gen, footprint_mb):
    """yields (name, the library's call, the torch restatement, bytes the kernel has to move) of the two calls, each over a
    ring of buffer sets that is freed before the next is made"""
    def sets(bytes_per_set):
        return max(2, -(-footprint_mb * 10 ** 6 // max(bytes_per_set, 1)))

    rate = 100.0 + 900.0 * torch.rand(n, device=DEV, generator=gen)
    ring = Ring(lambda i: (feature_rows(n, gen), torch.empty(n, 56, device=DEV)), sets(APPLY_BYTES * n))

    def hip_apply():
        feat, out = ring.next()
        filter3d.apply_forward(feat, rate, k, out=out)
    yield "apply", hip_apply, lambda: torch_apply(ring.next()[0], rate, k), APPLY_BYTES * n
    del ring
    torch.cuda.empty_cache()

    feat = feature_rows(n, gen)
    ring = Ring(lambda i: (torch.randn(n, 56, device=DEV, generator=gen), torch.empty(n, 56, device=DEV)), sets(BACKWARD_BYTES * n))

    def hip_backward():
        grad, out = ring.next()
        filter3d.apply_backward(grad, feat, rate, k, out=out)
    yield "backward", hip_backward, lambda: torch_backward(ring.next()[0], feat, rate, k), BACKWARD_BYTES * n
    del ring
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--rate-shapes", default=RATE_SHAPES, help="ROWSxVIEWS of the rate pass, comma separated")
    ap.add_argument("--rows", default=ROWS, help="row counts of apply and its backward, comma separated")
    ap.add_argument("--steps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=20, help="untimed calls of every leg")
    ap.add_argument("--repeats", type=int, default=5, help="alternating rounds")
    ap.add_argument("--footprint-mb", type=int, default=600, help="bytes the buffer sets of a leg hold together, at least")
    ap.add_argument("--workload", default="cfg3_headline")
    ap.add_argument("--skip-iteration", action="store_true")
    ap.add_argument("--rocprof", action="store_true", help="the kernels' own time by a rocprofv3 kernel trace of a child process")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    H.require_gpu("bench_filter3d.py")
    out = {"component": "3D smoothing filter: sampling rates, apply, its backward and training iteration, 1x MI355X",
           "method": f"harness.alternate: {a.warmup} warm calls per leg, {a.repeats} rounds of one {a.steps}-call window per leg between device "
                     f"events; every apply call on the next of enough buffer sets to hold {a.footprint_mb} MB",
           "rate_ms": {}, "apply_ms": {}, "notes": []}
    gen = torch.Generator(device=DEV).manual_seed(0)
    k = filter3d.filter_k(0.2, 1)
    shapes = [tuple(int(v) for v in shape.lower().split("x")) for shape in a.rate_shapes.split(",")]
    rows = [int(v) for v in a.rows.split(",")]

    def rate_leg(n, n_views):
        pc, mask = cloud(n, gen)
        views, rate = ring_views(n_views, gen), torch.empty(n, device=DEV)
        return (lambda: filter3d.sampling_rate(pc, mask, views, W, HH, NEAR, MARGIN, out=rate)), (lambda: torch_rate(pc, mask, views))

    if a.child:                 # rocprofv3 target: the rate at the first shape, the two apply calls at the first row count
        hip, _ = rate_leg(*shapes[0])
        for _ in range(a.warmup + a.steps):
            hip()
        torch.cuda.synchronize()
        for _, hip, _, _ in apply_legs(rows[0], k, gen, a.footprint_mb):
            for _ in range(a.warmup + a.steps):
                hip()
            torch.cuda.synchronize()
        return

    def trace(shape_arg, rows_arg):
        return H.rocprof_kernel_stats([os.path.abspath(__file__), "--rate-shapes", shape_arg, "--rows", rows_arg, "--steps", str(a.steps * a.repeats),
                                       "--warmup", str(a.warmup), "--footprint-mb", str(a.footprint_mb), "--child"], ("k_filter3d_",), seconds=240)

    def us(table, *parts):
        return round(sum(r["avg_us"] for name, r in table.items() if any(part in name for part in parts)), 3)

    for n, n_views in shapes:
        hip, tch = rate_leg(n, n_views)
        leg = H.alternate({"hip": hip, "torch": tch}, a.steps, a.warmup, a.repeats)
        leg["rows"], leg["views"], leg["pairs"] = n, n_views, n * n_views
        leg["torch_over_hip"] = round(leg["torch"]["median_ms"] / leg["hip"]["median_ms"], 3)
        leg["hip_pairs_per_s"] = round(n * n_views / (leg["hip"]["median_ms"] * 1e-3), 1)
        if a.rocprof:
            table = trace(f"{n}x{n_views}", str(rows[0]))
            leg["kernels_rocprofv3"] = {name: r for name, r in table.items() if "rate" in name or "fill" in name}
            leg["device_us"] = us(table, "k_filter3d_rate", "k_filter3d_fill")
        else:
            leg["device_us"] = "not measured"
        out["rate_ms"][f"{n}x{n_views}"] = leg
        torch.cuda.empty_cache()

    for n in rows:
        rec = {"rows": n, "features_mb": round(n * 224 / 1e6, 3)}
        for name, hip, tch, nbytes in apply_legs(n, k, gen, a.footprint_mb):
            leg = H.alternate({"hip": hip, "torch": tch}, a.steps, a.warmup, a.repeats)
            leg["bytes"] = nbytes
            leg["hbm_floor_ms"] = round(nbytes / HBM_BYTES_PER_S * 1e3, 5)
            leg["torch_over_hip"] = round(leg["torch"]["median_ms"] / leg["hip"]["median_ms"], 3)
            rec[name] = leg
        if a.rocprof:
            table = trace(f"{min(n, 1000)}x1", str(n))
            rec["kernels_rocprofv3"] = {name: r for name, r in table.items() if "apply" in name or "backward" in name}
            for name, part in (("apply", "k_filter3d_apply"), ("backward", "k_filter3d_backward")):
                rec[name]["device_us"] = us(table, part)
                rec[name]["device_over_hbm_floor"] = round(rec[name]["device_us"] / (rec[name]["hbm_floor_ms"] * 1e3), 3)
        else:
            for name in ("apply", "backward"):
                rec[name]["device_us"] = "not measured"
        out["apply_ms"][str(n)] = rec

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
        loss_fn = LossFunction(LossFunction.LossFunctionConfig())
        gt = torch.rand(3, s.height, s.width, device=DEV, generator=gen)
        # the rates of the workload's own camera and two beside it
        T = torch.eye(4, dtype=torch.float64).repeat(3, 1, 1)
        T[:, 0, 3] = torch.tensor([-0.2, 0.0, 0.2], dtype=torch.float64)
        views = filter3d.view_table(T, inp.camera_info.camera_intrinsics, device=DEV)
        rate = filter3d.sampling_rate(inp.point_cloud.detach(), inp.point_invalid_mask, views, s.width, s.height, NEAR, MARGIN)
        plain_features = inp.point_cloud_features

        def iteration(mode):
            def it():
                of.zero_grad(); op.zero_grad()
                inp.point_cloud_features = filter3d.apply(plain_features, rate, k) if mode == "filter" else plain_features
                img = rast(inp)[0].permute(2, 0, 1)
                loss_fn(img, gt, point_invalid_mask=inp.point_invalid_mask, pointcloud_features=plain_features,
                        clamp_predicted=True)[0].backward()
                of.step(); op.step()
                controller.refinement()
            return it
        rec = H.alternate({"filter": iteration("filter"), "none": iteration("none")}, a.steps, a.warmup, a.repeats)
        rec["filter_minus_none_ms"] = round(rec["filter"]["median_ms"] - rec["none"]["median_ms"], 5)
        rec["filter_over_none"] = round(rec["filter"]["median_ms"] / rec["none"]["median_ms"], 4)
        rec["workload"], rec["height"], rec["width"], rec["rows"] = a.workload, s.height, s.width, int(plain_features.shape[0])
        out["training_iteration_ms"] = rec

    def legs(doc, path=()):
        if isinstance(doc, dict) and "windows_ms" in doc:
            yield "/".join(path), doc
        elif isinstance(doc, dict):
            for key, value in doc.items():
                yield from legs(value, path + (key,))
    for name, leg in legs(out):
        if leg["max_ms"] > 1.5 * leg["min_ms"]:
            out["notes"].append(f"{name}: its windows span {leg['min_ms']} to {leg['max_ms']} ms ({leg['windows_ms']}): more than one "
                                "regime in one leg, so its median and the ratios made from it are not a steady-state figure")
    assert set(out) == set(KEYS)
    H.write_json(out, a.out)


if __name__ == "__main__":
    main()
