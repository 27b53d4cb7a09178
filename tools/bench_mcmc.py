#!/usr/bin/env python3
"""Measure fixed-budget densification (include/gs_mcmc.h, mcmc.py), on cuda:0:
  calls      at every --rows size (a random scene with 1 % dead rows and a tenth more rows free, growth 5 %): gs_mcmc_noise,
             gs_mcmc_regulariser and gs_mcmc_relocate beside the same rules written in torch operations on the same device (the
             regulariser through autograd, the relocation with torch.multinomial and a binomial table, as the paper's code has
             it).  A relocation edits the scene, so both of its legs restore the scene first; restore_only is that part alone.
  iteration  a whole training iteration at --workload (tools/bench_trainer_step.py's fused_in_place leg): density="mcmc" --
             no hook, the regulariser's gradient before the optimiser steps and the noise behind them -- beside "adaptive": the
             controller's update as the backward hook and its refinement() behind the steps, inside its warm-up.  A relocation
             runs every hundredth iteration and is in neither leg: a hundredth of its time above is its share.
Each comparison alternates its legs in one process (harness.alternate: every leg warmed, then `repeats` rounds of one timed
window per leg, a window being `--steps` calls between two device events).  No ratio is asserted.

    python tools/bench_mcmc.py [--out profiles/mcmc_bench.json] [--rows 500000,2000000] [--steps N] [--warmup N] [--repeats N]
                               [--workload cfg3_headline] [--skip-iteration]
"""
import argparse
import math
from types import SimpleNamespace

import harness as H
import numpy as np
import torch

from taichi_3d_gaussian_splatting_amd import mcmc

DEV = "cuda:0"
ROWS = "500000,2000000"
KEYS = ("component", "method", "calls_ms", "training_iteration_ms", "notes")


def random_scene(n_valid, seed=0, dead_share=0.01, free_share=0.1):
    """-> (scene of n_valid valid rows, dead_share of them below the opacity threshold, and free_share more rows free; numpy copies)"""
    rng = np.random.default_rng(seed)
    n = n_valid + int(n_valid * free_share)
    ft = rng.normal(0.0, 0.5, (n, 56)).astype(np.float32)
    ft[:, 4:7] = rng.normal(-4.0, 0.5, (n, 3)).astype(np.float32)
    ft[:, 7] = rng.normal(0.0, 2.0, n).astype(np.float32)
    ft[rng.random(n) < dead_share, 7] = -7.0
    mask = np.zeros(n, np.int8)
    mask[n_valid:] = 1
    return SimpleNamespace(point_cloud=torch.tensor(rng.normal(0.0, 1.0, (n, 3)).astype(np.float32), device=DEV),
                           point_cloud_features=torch.tensor(ft, device=DEV), point_invalid_mask=torch.tensor(mask, device=DEV),
                           point_object_id=torch.zeros(n, dtype=torch.int32, device=DEV))


# ---- the same rules in torch operations ------------------------------------------------------------------------------------
def torch_rotation(q):
    x, y, z, w = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                        2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)


def torch_noise(scene, noise_scale):
    pc, ft, valid = scene.point_cloud, scene.point_cloud_features, scene.point_invalid_mask == 0
    gate = torch.sigmoid(mcmc.GATE_K * ((1 - torch.sigmoid(ft[:, 7])) - mcmc.GATE_X0))
    R = torch_rotation(ft[:, 0:4])
    RS = R * torch.exp(ft[:, 4:7])[:, None, :]
    Sigma = torch.bmm(RS, RS.transpose(1, 2))
    delta = torch.bmm(Sigma, (torch.randn_like(pc) * (gate * noise_scale)[:, None])[:, :, None])[:, :, 0]
    pc += torch.where(valid[:, None] & torch.isfinite(delta).all(1, keepdim=True), delta, torch.zeros_like(delta))


def torch_regulariser(scene, lambda_opacity, lambda_scale, grad):
    ft = scene.point_cloud_features.detach().requires_grad_(True)
    valid = scene.point_invalid_mask == 0
    value = lambda_opacity * torch.sigmoid(ft[valid, 7]).mean() + lambda_scale * torch.exp(ft[valid, 4:7]).mean()
    value.backward()
    grad += ft.grad
    return value.detach()


_BINOMS = None


def torch_relocate(scene, moments, config, cap):
    """the paper's code in torch: dead rows and the growth sampled with torch.multinomial over the opacities of the live rows
    (two rounds), the new opacity and scale from a binomial table, moments of the sources zeroed.  It reads counts on the host."""
    global _BINOMS
    n_max = config.n_max
    if _BINOMS is None:
        _BINOMS = torch.tensor([[math.comb(i, k) if k <= i else 0 for k in range(n_max)] for i in range(n_max)], dtype=torch.float64, device=DEV)
    pc, ft, mask, obj = scene.point_cloud, scene.point_cloud_features, scene.point_invalid_mask, scene.point_object_id
    k = torch.arange(n_max, device=DEV, dtype=torch.float64)
    sign_over_root = torch.where(k.long() % 2 == 0, 1.0, -1.0) / torch.sqrt(k + 1)

    def copy_onto(dest):
        if dest.numel() == 0:
            return
        alive = torch.nonzero((mask == 0) & (ft[:, 7] > mcmc.min_opacity_logit(config.min_opacity)))[:, 0]
        opacity = torch.sigmoid(ft[alive, 7])
        src = alive[torch.multinomial(opacity, dest.numel(), replacement=True)]
        M = torch.clamp(torch.bincount(src, minlength=pc.shape[0])[src] + 1, max=n_max)
        o = torch.sigmoid(ft[src, 7]).double()
        p = torch.clamp(1 - (1 - o) ** (1.0 / M), 0.005, 1 - 2.0 ** -24)
        powers = p[:, None] ** (k + 1)[None, :]                                       # (D, n_max)
        inner = torch.cumsum(torch.ones(n_max, n_max, device=DEV, dtype=torch.float64), 0)   # row i: i + 1
        table = (_BINOMS * sign_over_root[None, :])                                   # (i, k)
        per_i = powers @ table.T                                                      # (D, n_max): sum over k for every i
        d = (per_i * (inner[:, 0][None, :] <= M[:, None])).sum(1)
        new_logit = torch.log(p / (1 - p)).float()
        new_scale = (ft[src, 4:7].double() + torch.log(o / d)[:, None]).float()
        ft[src, 7], ft[src, 4:7] = new_logit, new_scale
        ft[dest], pc[dest], obj[dest], mask[dest] = ft[src], pc[src], obj[src], 0
        for m in moments:
            m[src] = 0
    with torch.no_grad():
        copy_onto(torch.nonzero((mask == 0) & ~(ft[:, 7] > mcmc.min_opacity_logit(config.min_opacity)))[:, 0])
        valid = int((mask == 0).sum())
        n_new = max(0, min(cap, valid + valid * config.grow_permille // 1000) - valid)
        copy_onto(torch.nonzero(mask == 1)[:n_new, 0])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--rows", default=ROWS, help="valid rows of the scenes of the three calls, comma separated")
    ap.add_argument("--steps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=20, help="untimed calls of every leg")
    ap.add_argument("--repeats", type=int, default=5, help="alternating rounds")
    ap.add_argument("--workload", default="cfg3_headline")
    ap.add_argument("--skip-iteration", action="store_true")
    a = ap.parse_args()
    H.require_gpu("bench_mcmc.py")
    config = mcmc.MCMCConfig()
    noise_scale = config.noise_lr * 1.6e-4
    out = {"component": "fixed-budget densification: noise, regulariser, relocation and training iteration, 1x MI355X",
           "method": f"harness.alternate: {a.warmup} warm calls per leg, {a.repeats} rounds of one {a.steps}-call window per leg between device events",
           "calls_ms": {}, "notes": []}
    for n_valid in [int(v) for v in a.rows.split(",")]:
        scene = random_scene(n_valid)
        n = scene.point_cloud.shape[0]
        grad = torch.zeros_like(scene.point_cloud_features)
        step = [0]

        def hip_noise():
            step[0] += 1
            mcmc.inject_noise(scene, noise_scale, step[0])
        rec = {"rows_valid": n_valid, "rows_allocated": n}
        rec["noise"] = H.alternate({"hip": hip_noise, "torch": lambda: torch_noise(scene, noise_scale)}, a.steps, a.warmup, a.repeats)
        rec["regulariser"] = H.alternate({"hip": lambda: mcmc.add_regulariser_grad(scene, config.opacity_reg, config.scale_reg, grad=grad),
                                          "torch_autograd": lambda: torch_regulariser(scene, config.opacity_reg, config.scale_reg, grad)},
                                         a.steps, a.warmup, a.repeats)
        saved = [t.clone() for t in (scene.point_cloud, scene.point_cloud_features, scene.point_invalid_mask, scene.point_object_id)]
        moments = [torch.ones_like(scene.point_cloud_features), torch.ones_like(scene.point_cloud_features),
                   torch.ones_like(scene.point_cloud), torch.ones_like(scene.point_cloud)]
        optimizers = (SimpleNamespace(params=[scene.point_cloud_features], state=[dict(exp_avg=moments[0], exp_avg_sq=moments[1])]),
                      SimpleNamespace(params=[scene.point_cloud], state=[dict(exp_avg=moments[2], exp_avg_sq=moments[3])]))
        plan = mcmc.MCMCPlan(n, DEV)

        def restore():
            for t, s in zip((scene.point_cloud, scene.point_cloud_features, scene.point_invalid_mask, scene.point_object_id), saved):
                t.copy_(s)

        def hip_relocate():
            restore()
            mcmc.relocate(scene, config, optimizers, 0, plan)

        def torch_relocate_leg():
            restore()
            torch_relocate(scene, moments, config, n)
        hip_relocate()
        rec["relocate_counts"] = dict(zip(mcmc.COUNTS, (int(x) for x in plan.counts.cpu())))
        rec["relocate"] = H.alternate({"hip": hip_relocate, "torch": torch_relocate_leg, "restore_only": restore},
                                      max(a.steps // 4, 1), max(a.warmup // 4, 1), a.repeats)
        restore()
        for name, other in (("noise", "torch"), ("regulariser", "torch_autograd"), ("relocate", "torch")):
            rec[name]["torch_over_hip"] = round(rec[name][other]["median_ms"] / rec[name]["hip"]["median_ms"], 3)
        out["calls_ms"][str(n_valid)] = rec
        del scene, grad, saved, moments, plan
        torch.cuda.empty_cache()

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
        scene = SimpleNamespace(point_cloud=inp.point_cloud, point_cloud_features=inp.point_cloud_features,
                                point_invalid_mask=inp.point_invalid_mask, point_object_id=inp.point_object_id)
        controller_config = GaussianPointAdaptiveController.GaussianPointAdaptiveControllerConfig()
        controller_config.num_iterations_warm_up = 10 ** 9
        controller = GaussianPointAdaptiveController(
            config=controller_config, maintained_parameters=GaussianPointAdaptiveController.GaussianPointAdaptiveControllerMaintainedParameters(
                pointcloud=inp.point_cloud, pointcloud_features=inp.point_cloud_features, point_invalid_mask=inp.point_invalid_mask,
                point_object_id=inp.point_object_id), seed=0)
        rasts = {"adaptive": Rast(Rast.GaussianPointCloudRasterisationConfig(), backward_valid_point_hook=controller.update),
                 "mcmc": Rast(Rast.GaussianPointCloudRasterisationConfig())}
        of, op = FusedAdam([inp.point_cloud_features], lr=1e-3), FusedAdam([inp.point_cloud], lr=1e-5)
        strategy = mcmc.MCMCStrategy(mcmc.MCMCConfig(refine_start=10 ** 9), scene, of, op)
        loss_fn = LossFunction(LossFunction.LossFunctionConfig())
        gt = torch.rand(3, s.height, s.width, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0))
        count = [0]

        def iteration(density):
            def it():
                count[0] += 1
                of.zero_grad(); op.zero_grad()
                img, _, _ = rasts[density](inp)
                loss_fn(img.permute(2, 0, 1), gt, point_invalid_mask=inp.point_invalid_mask, pointcloud_features=inp.point_cloud_features,
                        clamp_predicted=True)[0].backward()
                if density == "mcmc":
                    strategy.before_step(count[0])
                of.step(); op.step()
                if density == "mcmc":
                    strategy.after_step(count[0], op.lr)
                else:
                    controller.refinement()
            return it
        rec = H.alternate({"mcmc": iteration("mcmc"), "adaptive": iteration("adaptive")}, a.steps, a.warmup, a.repeats)
        rec["mcmc_over_adaptive"] = round(rec["mcmc"]["median_ms"] / rec["adaptive"]["median_ms"], 4)
        rec["workload"] = a.workload
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
