#!/usr/bin/env python3
"""Measure camera pose refinement (include/gs_pose_table.h, pose_table.py), on cuda:0:
  call       gs_pose_compose and gs_pose_compose_backward at V = 1, K = 1 as the trainer calls them (a table row, the gradient
             written into the table), beside the same formulas in torch operations with autograd (quaternion product, rotation,
             backward) on the same device.  These are latency-bound single-wave launches: a window holds the host's share of a
             call too; with --rocprof the kernels' own time is taken from a rocprofv3 kernel trace of a child process that makes
             the same calls, in a run of its own.
  corrected  PoseTable.corrected over --views views in one launch.
  iteration  a whole training iteration at --workload with the view's pose refined (compose, the rasteriser's pose gradient --
             k_pose_points and k_pose_reduce --, compose's backward, one more Adam step) beside the iteration as it is.
  margins    with --margins-out: the three seeded runs of tests/test_gpu_trainer_poses.py on planted pose noise, written to that
             file (profiles/pose_refine_margins.json).
Each comparison alternates its legs in one process (harness.alternate).  No ratio is asserted.

    python tools/bench_poses.py [--out profiles/pose_refine_bench.json] [--steps N] [--warmup N] [--repeats N] [--views 300]
                                [--workload cfg3_headline] [--skip-iteration] [--rocprof] [--margins-out profiles/pose_refine_margins.json]
"""
import argparse
import os
import tempfile

import harness as H
import torch

from taichi_3d_gaussian_splatting_amd import pose_table

DEV = "cuda:0"
KEYS = ("component", "method", "launches", "call_ms", "corrected_ms", "training_iteration_ms", "notes")


def torch_compose(q, t, delta):
    """the header's closed form in torch operations, one view: q (K,4), t (K,3), delta (6,) -> (q', t')"""
    w, u = delta[:3], delta[3:]
    th = w.norm()
    dq = torch.cat([w * (torch.sin(th / 2) / th), torch.cos(th / 2)[None]])
    x0, y0, z0, w0 = q.unbind(-1)
    x1, y1, z1, w1 = dq.unbind(-1)
    q_out = torch.stack([w0 * x1 + x0 * w1 + y0 * z1 - z0 * y1, w0 * y1 - x0 * z1 + y0 * w1 + z0 * x1,
                         w0 * z1 + x0 * y1 - y0 * x1 + z0 * w1, w0 * w1 - x0 * x1 - y0 * y1 - z0 * z1], dim=-1)
    R = torch.stack([1 - 2 * (y0 * y0 + z0 * z0), 2 * (x0 * y0 - w0 * z0), 2 * (x0 * z0 + w0 * y0),
                     2 * (x0 * y0 + w0 * z0), 1 - 2 * (x0 * x0 + z0 * z0), 2 * (y0 * z0 - w0 * x0),
                     2 * (x0 * z0 - w0 * y0), 2 * (y0 * z0 + w0 * x0), 1 - 2 * (x0 * x0 + y0 * y0)], dim=-1).reshape(-1, 3, 3)
    return q_out, t + R @ u


def call_legs(gen):
    """-> {name: fn}: forward and forward + backward + Adam step of one view, the library's and torch's"""
    table = pose_table.PoseTable(4, DEV, pose_table.PoseRefinementConfig(num_iterations=10 ** 6))
    table.delta.copy_(torch.randn(4, 6, device=DEV, generator=gen) * 0.01)
    q = torch.nn.functional.normalize(torch.randn(1, 4, device=DEV, generator=gen), dim=1)
    t = torch.randn(1, 3, device=DEV, generator=gen)
    gq, gt = torch.randn(1, 4, device=DEV, generator=gen), torch.randn(1, 3, device=DEV, generator=gen)
    free = table.delta[1].clone().requires_grad_(True)
    adam = torch.optim.Adam([free], lr=1e-3)
    q3, t3, d2 = q[None].contiguous(), t[None].contiguous(), table.delta[1:2]
    gq3, gt3, out = gq[None].contiguous(), gt[None].contiguous(), torch.empty(1, 6, device=DEV)

    def hip_forward():
        pose_table.compose_forward(q3, t3, d2)

    def hip_backward():
        pose_table.compose_backward(q3, d2, gq3, gt3, 1e-6, grad_delta=out)

    def hip_step():
        qc, tc = pose_table.compose(q, t, table.row(1))
        torch.autograd.backward([qc, tc], [gq, gt])
        table.step(1, 0)

    def torch_forward():
        with torch.no_grad():
            torch_compose(q, t, free)

    def torch_step():
        adam.zero_grad(set_to_none=True)
        qc, tc = torch_compose(q, t, free)
        torch.autograd.backward([qc, tc], [gq, gt])
        adam.step()
    return {"hip_forward": hip_forward, "hip_backward": hip_backward, "hip_step": hip_step, "torch_forward": torch_forward, "torch_step": torch_step}


def margins(path):
    import pose_trainer_util as PU
    with tempfile.TemporaryDirectory(prefix="pose_margins_") as root:
        doc = PU.planted_noise_runs(root, DEV)["margins"]
    doc = {k: (round(v, 6) if isinstance(v, float) else v) for k, v in doc.items()}
    doc["run"] = "tests/pose_trainer_util.py: planted_noise_runs, three runs from the perturbed scene on the arc views"
    H.write_json(doc, path)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--steps", type=int, default=200, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=50, help="untimed calls of every leg")
    ap.add_argument("--repeats", type=int, default=5, help="alternating rounds")
    ap.add_argument("--views", type=int, default=300, help="views of the corrected() leg")
    ap.add_argument("--workload", default="cfg3_headline")
    ap.add_argument("--iteration-steps", type=int, default=20, help="iterations per timed window of the training-iteration legs")
    ap.add_argument("--skip-iteration", action="store_true")
    ap.add_argument("--rocprof", action="store_true", help="the kernels' own time by a rocprofv3 kernel trace of a child process")
    ap.add_argument("--margins-out", help="also make the three training runs on planted noise and write their figures here")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    H.require_gpu("bench_poses.py")
    gen = torch.Generator(device=DEV).manual_seed(0)
    legs = call_legs(gen)
    if a.child:                 # rocprofv3 target: the two launches at V = 1, K = 1
        for name in ("hip_forward", "hip_backward"):
            for _ in range(a.warmup + a.steps):
                legs[name]()
            torch.cuda.synchronize()
        return
    out = {"component": "camera pose refinement: compose and its backward at V = 1, K = 1, all views in one launch, training iteration, 1x MI355X",
           "method": f"harness.alternate: {a.warmup} warm calls per leg, {a.repeats} rounds of one {a.steps}-call window per leg between device "
                     "events (host side of a call included)",
           "launches": {"compose": 1, "compose_backward": 1, "adam_step": 1}, "notes": []}
    out["call_ms"] = H.alternate(legs, a.steps, a.warmup, a.repeats)
    out["call_ms"]["torch_step_over_hip_step"] = round(out["call_ms"]["torch_step"]["median_ms"] / out["call_ms"]["hip_step"]["median_ms"], 3)
    if a.rocprof:
        out["call_ms"]["kernels_rocprofv3"] = H.rocprof_kernel_stats(
            [os.path.abspath(__file__), "--steps", str(a.steps), "--warmup", str(a.warmup), "--child"], ("k_pose_compose",), seconds=300)
    else:
        out["call_ms"]["kernels_rocprofv3"] = "not measured"

    table = pose_table.PoseTable(a.views, DEV)
    table.delta.copy_(torch.randn(a.views, 6, device=DEV, generator=gen) * 0.01)
    qv = torch.nn.functional.normalize(torch.randn(a.views, 4, device=DEV, generator=gen), dim=1)
    tv = torch.randn(a.views, 3, device=DEV, generator=gen)
    out["corrected_ms"] = dict(H.alternate({"hip": lambda: table.corrected(qv, tv)}, a.steps, a.warmup, a.repeats), views=a.views)

    if a.skip_iteration:
        out["training_iteration_ms"] = "not measured"
    else:
        import dataclasses
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
        loss_fn = LossFunction(LossFunction.LossFunctionConfig())
        gt = torch.rand(3, s.height, s.width, device=DEV, generator=gen)
        poses = pose_table.PoseTable(4, DEV, pose_table.PoseRefinementConfig(lr=1e-6, lr_final=1e-7, num_iterations=10 ** 6))
        q_base, t_base = inp.q_pointcloud_camera, inp.t_pointcloud_camera

        def iteration(refined):
            def it():
                of.zero_grad(); op.zero_grad()
                step_input = inp
                if refined:
                    qc, tc = pose_table.compose(q_base, t_base, poses.row(1))
                    step_input = dataclasses.replace(inp, q_pointcloud_camera=qc, t_pointcloud_camera=tc)
                image = rast(step_input)[0]
                loss = loss_fn(image.permute(2, 0, 1), gt, point_invalid_mask=inp.point_invalid_mask, pointcloud_features=inp.point_cloud_features,
                               clamp_predicted=True)[0]
                loss.backward()
                of.step(); op.step()
                if refined:
                    poses.step(1, 0)
                controller.refinement()
            return it
        rec = H.alternate({"refined": iteration(True), "none": iteration(False)}, a.iteration_steps, min(a.warmup, 20), a.repeats)
        rec["refined_minus_none_ms"] = round(rec["refined"]["median_ms"] - rec["none"]["median_ms"], 5)
        rec["refined_over_none"] = round(rec["refined"]["median_ms"] / rec["none"]["median_ms"], 4)
        rec["workload"], rec["height"], rec["width"] = a.workload, s.height, s.width
        out["training_iteration_ms"] = rec
        out["notes"].append("training_iteration_ms: the difference holds the rasteriser's pose gradient (k_pose_points, k_pose_reduce) beside the "
                            "three launches of the table")

    def timed(doc, path=()):
        if isinstance(doc, dict) and "windows_ms" in doc:
            yield "/".join(path), doc
        elif isinstance(doc, dict):
            for k, v in doc.items():
                yield from timed(v, path + (k,))
    for name, leg in timed(out):
        if leg["max_ms"] > 1.5 * leg["min_ms"]:
            out["notes"].append(f"{name}: its windows span {leg['min_ms']} to {leg['max_ms']} ms ({leg['windows_ms']}): more than one "
                                "regime in one leg, so its median and the ratios made from it are not a steady-state figure")
    assert set(out) == set(KEYS)
    H.write_json(out, a.out)
    if a.margins_out:
        margins(a.margins_out)


if __name__ == "__main__":
    main()
