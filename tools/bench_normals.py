#!/usr/bin/env python3
"""Measure the Gaussian normals and the normal-consistency term (include/gs_normals.h, normals.py), on cuda:0:
  kernels    at every --sizes image: gs_normal_consistency_forward / _backward (max_rel_jump 0.1, min_length 0.5, a pixel weight) as
             the trainer calls them, beside the same formulas in torch operations on the same device (float32 planes, float64
             sums; the torch backward leg is the forward and autograd's backward through it).  Every call takes the next of
             enough buffer sets to hold more than --footprint-mb, as tools/bench_geometry.py does, so that the planes come from
             HBM; each call's bytes stand beside the time they take at 6.3 TB/s (hbm_floor_ms).  With --rocprof the kernels' own
             time comes from a rocprofv3 kernel trace of a child process that makes the same calls, in a run of its own.
  rows       at every --rows count: gs_gaussian_normals_forward / _backward beside the same formulas in torch operations.
  iteration  a whole training iteration at --workload with the term (rendered normals over the step's frame: the per-row kernel,
             the three-channel blend forward and backward, the consistency forward and backward, the depth backward) beside one
             without, and the split of the difference where --rocprof gives the kernels' times.
Each comparison alternates its legs in one process (harness.alternate).  No ratio is asserted.

    python tools/bench_normals.py [--out profiles/normal_consistency_bench.json] [--sizes 1920x1088,976x544] [--rows 500000,2000000]
                                  [--steps N] [--warmup N] [--repeats N] [--workload cfg3_headline] [--skip-iteration] [--rocprof]
"""
import argparse
import os

import bench_geometry as BG
import harness as H
import torch

from taichi_3d_gaussian_splatting_amd import geometry, normals

DEV = BG.DEV
KEYS = ("component", "method", "launches", "kernels_ms", "rows_ms", "training_iteration_ms", "notes")
JUMP, MIN_LENGTH = 0.1, 0.5
KERNELS = ("k_normal_consistency", "k_geometry_finish", "k_gaussian_normals", "k_channels")


def torch_consistency(D, R, w_p, K, backward):
    if backward:
        D, R = D.detach().requires_grad_(True), R.detach().requires_grad_(True)
    ok, c, length = BG.torch_normals(D, K, JUMP)
    m = R[1:-1, 1:-1].permute(2, 0, 1)
    k = (m * m).sum(0).sqrt()
    w = torch.clamp(w_p[1:-1, 1:-1], min=0)
    sel = ok & (k >= MIN_LENGTH) & (w > 0)
    cos = ((c / length) * (m / torch.where(sel, k, torch.ones_like(k)))).sum(0)
    zero = torch.zeros_like(cos)
    loss = (torch.where(sel, w * (1.0 - cos), zero).sum(dtype=torch.float64) / torch.where(sel, w, zero).sum(dtype=torch.float64)).float()
    if backward:
        loss.backward()
        return loss, D.grad, R.grad
    return loss


def torch_rotation(q):
    x, y, z, w = q.unbind(-1)
    return torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                        torch.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                        torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def torch_gaussian_normals(pc, f, q_pc, t_pc, g=None):
    """the header's normal in float32 torch operations (one object); with g: also the gradient to f by autograd"""
    if g is not None:
        f = f.detach().requires_grad_(True)
    k = f[:, 4:7].argmin(dim=1)
    c = torch_rotation(f[:, :4]).gather(2, k[:, None, None].expand(-1, 3, 1))[:, :, 0]
    u = c / c.norm(dim=1, keepdim=True)
    P = torch_rotation(q_pc[0])
    m, p = u @ P, (pc - t_pc[0]) @ P
    n = torch.where(((m * p).sum(1) <= 0)[:, None], m, -m)
    if g is not None:
        (n * g).sum().backward()
        return n, f.grad
    return n


def consistency_legs(Hh, W, gen, footprint_mb):
    plane = Hh * W * 4
    K = BG.camera(Hh, W)

    def make(i):
        yy, xx = torch.meshgrid(torch.arange(Hh, device=DEV, dtype=torch.float32), torch.arange(W, device=DEV, dtype=torch.float32), indexing="ij")
        D = 3.0 + 0.3 * torch.sin(xx / 37.0 + i) + 0.2 * torch.cos(yy / 23.0) + 0.002 * torch.rand(Hh, W, device=DEV, generator=gen)
        D = torch.where(torch.rand(Hh, W, device=DEV, generator=gen) < 0.02, torch.zeros_like(D), D)          # holes
        R = torch.randn(Hh, W, 3, device=DEV, generator=gen) * 0.2 + torch.tensor([0.0, 0.0, -1.0], device=DEV)
        R = R / R.norm(dim=2, keepdim=True) * (0.3 + 0.7 * torch.rand(Hh, W, 1, device=DEV, generator=gen))     # a third below min_length
        w_p = torch.rand(Hh, W, device=DEV, generator=gen)
        return dict(D=D.contiguous(), R=R.contiguous(), w_p=w_p, gd=torch.empty(Hh, W, device=DEV), gr=torch.empty(Hh, W, 3, device=DEV),
                    t=torch.empty(geometry.LOSS_TERMS, device=DEV))

    ring = BG.Ring(make, BG.sets_for(footprint_mb, 10 * plane))
    for s in ring.sets:                     # the backward reads the terms the forward wrote
        normals.normal_consistency_forward(s["D"], s["R"], K, s["w_p"], JUMP, MIN_LENGTH, terms=s["t"])

    def forward():
        s = ring.next()
        normals.normal_consistency_forward(s["D"], s["R"], K, s["w_p"], JUMP, MIN_LENGTH, terms=s["t"])

    def backward():
        s = ring.next()
        normals.normal_consistency_backward(s["D"], s["R"], K, s["w_p"], JUMP, MIN_LENGTH, s["t"], out_depth=s["gd"], out_rendered=s["gr"])

    def torch_leg(back):
        def leg():
            s = ring.next()
            return torch_consistency(s["D"], s["R"], s["w_p"], K, back)
        return leg
    yield "normal_consistency_forward", forward, torch_leg(False), 5 * plane            # D, 3 of R, w_p
    yield "normal_consistency_backward", backward, torch_leg(True), 9 * plane          # and grad_D, 3 of grad_R
    del ring
    torch.cuda.empty_cache()


def row_legs(n, gen):
    pc = torch.randn(n, 3, device=DEV, generator=gen)
    f = torch.randn(n, normals.FEATURES, device=DEV, generator=gen)
    q_pc = torch.tensor([[0.1, -0.2, 0.05, 0.97]], device=DEV)
    q_pc = q_pc / q_pc.norm()
    t_pc = torch.tensor([[0.0, 0.0, -5.0]], device=DEV)
    g = torch.randn(n, 3, device=DEV, generator=gen)
    out_n, out_g = torch.empty(n, 3, device=DEV), torch.empty(n, normals.FEATURES, device=DEV)
    yield ("gaussian_normals_forward", lambda: normals.gaussian_normals_forward(pc, f, q_pc, t_pc, None, out=out_n),
           lambda: torch_gaussian_normals(pc, f, q_pc, t_pc), n * 4 * (10 + 3))                      # q, log s, x in; n out
    yield ("gaussian_normals_backward", lambda: normals.gaussian_normals_backward(pc, f, q_pc, t_pc, None, g, out=out_g),
           lambda: torch_gaussian_normals(pc, f, q_pc, t_pc, g), n * 4 * (10 + 3 + normals.FEATURES))


def training_iteration(a, gen):
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
    for mode in ("consistency", "none"):
        cfg = Rast.GaussianPointCloudRasterisationConfig()
        cfg.differentiable_depth = mode == "consistency"
        rast[mode] = Rast(cfg, backward_valid_point_hook=controller.update)
    of, op = FusedAdam([inp.point_cloud_features], lr=1e-3), FusedAdam([inp.point_cloud], lr=1e-5)
    loss_fn = LossFunction(LossFunction.LossFunctionConfig())
    gt = torch.rand(3, s.height, s.width, device=DEV, generator=gen)
    K = geometry.intrinsics_tuple(torch.as_tensor(s.camera_intrinsics))
    tensors, pose = (inp.point_cloud, inp.point_cloud_features, inp.point_object_id), (inp.q_pointcloud_camera, inp.t_pointcloud_camera)

    def iteration(mode):
        def it():
            of.zero_grad(); op.zero_grad()
            image, image_depth, _ = rast[mode](inp)
            loss = loss_fn(image.permute(2, 0, 1), gt, point_invalid_mask=inp.point_invalid_mask, pointcloud_features=inp.point_cloud_features,
                           clamp_predicted=True)[0]
            if mode == "consistency":
                rendered = normals.rendered_normals(rast[mode], tensors, pose)
                loss = loss + 0.05 * normals.normal_consistency_checked(image_depth, rendered, K, None, JUMP, MIN_LENGTH)
            loss.backward()
            of.step(); op.step()
            controller.refinement()
        return it
    if a.child:
        for _ in range(a.warmup + a.steps):
            iteration("consistency")()
        torch.cuda.synchronize()
        return None
    rec = H.alternate({"consistency": iteration("consistency"), "none": iteration("none")}, a.steps, a.warmup, a.repeats)
    rec["consistency_minus_none_ms"] = round(rec["consistency"]["median_ms"] - rec["none"]["median_ms"], 5)
    rec["consistency_over_none"] = round(rec["consistency"]["median_ms"] / rec["none"]["median_ms"], 4)
    rec["workload"], rec["height"], rec["width"] = a.workload, s.height, s.width
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--sizes", default=BG.SIZES, help="WxH of the images, comma separated")
    ap.add_argument("--rows", default="500000,2000000", help="row counts of the per-row kernels, comma separated")
    ap.add_argument("--steps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=20, help="untimed calls of every leg")
    ap.add_argument("--repeats", type=int, default=5, help="alternating rounds")
    ap.add_argument("--footprint-mb", type=int, default=600, help="bytes the buffer sets of a size hold together, at least")
    ap.add_argument("--workload", default="cfg3_headline")
    ap.add_argument("--skip-iteration", action="store_true")
    ap.add_argument("--rocprof", action="store_true", help="the kernels' own time by a rocprofv3 kernel trace of a child process")
    ap.add_argument("--child", choices=("kernels", "iteration"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    H.require_gpu("bench_normals.py")
    out = {"component": "Gaussian normals and normal consistency: per-row kernels, consistency forward and backward, training iteration, 1x MI355X",
           "method": f"harness.alternate: {a.warmup} warm calls per leg, {a.repeats} rounds of one {a.steps}-call window per leg between device "
                     f"events; every image call on the next of enough buffer sets to hold {a.footprint_mb} MB",
           "launches": {"forward": normals.FORWARD_LAUNCHES, "backward": normals.BACKWARD_LAUNCHES, "gaussian_normals": 1},
           "kernels_ms": {}, "rows_ms": {}, "notes": []}
    gen = torch.Generator(device=DEV).manual_seed(0)
    sizes = [tuple(int(v) for v in s.lower().split("x")) for s in a.sizes.split(",") if s]          # ("": none, as the traced children ask)
    rows = [int(v) for v in a.rows.split(",") if v]
    if a.child == "kernels":                # rocprofv3 target: every library leg at every size and row count
        for legs in [consistency_legs(Hh, W, gen, a.footprint_mb) for W, Hh in sizes] + [row_legs(n, gen) for n in rows]:
            for _, hip, _, _ in legs:           # (a generator: its buffers live while its legs are being called)
                for _ in range(a.warmup + a.steps):
                    hip()
                torch.cuda.synchronize()
        return
    if a.child == "iteration":
        training_iteration(a, gen)
        return

    def measure(name, hip, tch, nbytes):
        leg = H.alternate({"hip": hip, "torch": tch}, a.steps, a.warmup, a.repeats)
        leg["bytes"] = nbytes
        leg["hbm_floor_ms"] = round(nbytes / BG.HBM_BYTES_PER_S * 1e3, 5)
        leg["torch_over_hip"] = round(leg["torch"]["median_ms"] / leg["hip"]["median_ms"], 3)
        return leg

    def traced(child, extra, seconds=300):
        return H.rocprof_kernel_stats([os.path.abspath(__file__), "--steps", str(a.steps * a.repeats), "--warmup", str(a.warmup), "--footprint-mb",
                                       str(a.footprint_mb), "--workload", a.workload, "--child", child] + extra, KERNELS, seconds=seconds)
    for W, Hh in sizes:
        rec = {"height": Hh, "width": W, "plane_mb": round(Hh * W * 4 / 1e6, 3)}
        for name, hip, tch, nbytes in consistency_legs(Hh, W, gen, a.footprint_mb):
            rec[name] = measure(name, hip, tch, nbytes)
        rec["kernels_rocprofv3"] = traced("kernels", ["--sizes", f"{W}x{Hh}", "--rows", ""]) if a.rocprof else "not measured"
        out["kernels_ms"][f"{W}x{Hh}"] = rec
    for n in rows:
        rec = {"rows": n}
        for name, hip, tch, nbytes in row_legs(n, gen):
            rec[name] = measure(name, hip, tch, nbytes)
        rec["kernels_rocprofv3"] = traced("kernels", ["--sizes", "", "--rows", str(n)]) if a.rocprof else "not measured"
        out["rows_ms"][str(n)] = rec
    if a.skip_iteration:
        out["training_iteration_ms"] = "not measured"
    else:
        rec = training_iteration(a, gen)
        # the split of the difference: the term's own kernels, the three-channel blend and the rest (the depth backward)
        rec["kernels_rocprofv3"] = traced("iteration", []) if a.rocprof else "not measured"
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
