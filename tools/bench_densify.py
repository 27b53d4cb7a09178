#!/usr/bin/env python3
"""Measure one densification (gs_density_select + gs_density_apply) on cuda:0 against the torch restatement of the
reference's _find_densify_points / _add_densify_points (tests/density_ref.py, CTRL:170-353, with a torch Philox draw
in place of its Taichi sampling kernel), both timed with device events around the whole step, host syncs included.

Scene: 1e6 rows, 5e5 of them valid (scene_io.preallocate(..., 2.0)); the hook of one view with 2e5 in-camera points;
thresholds chosen from the data so that about 5 % of the valid rows densify and about 1 % are pruned.
The timer is this tool's own: the scene is restored and the device drained before every repetition, so each event pair
brackets one step on an idle GPU.  Prints one JSON line and writes it to profiles/density_bench.json (or the path given
as the first argument or as --out).

    python tools/bench_densify.py [PATH] [--rows 500000] [--in-camera 200000] [--steps 20] [--warmup 3] [--out PATH]
"""
import argparse
import os
import types

import harness as H
import numpy as np
import torch

from density_ref import add_densify_points, find_densify_points
from taichi_3d_gaussian_splatting_amd import GaussianPointAdaptiveController as Ctl
from taichi_3d_gaussian_splatting_amd.scene_io import preallocate
from taichi_3d_gaussian_splatting_amd.synthetic import synth


def make_workload(N_VALID, M):
    s = synth(N_VALID, 1920, 1080, 0.02, sh_deg=3, seed=0)
    pc, ft, mask, obj = preallocate(s.point_cloud, s.point_cloud_features, 2.0)
    N = pc.shape[0]
    rng = np.random.default_rng(1)
    ids = np.sort(rng.choice(N_VALID, M, replace=False)).astype(np.int32)
    npix = rng.integers(0, 2000, M).astype(np.int32)
    depth = rng.uniform(2, 10, M).astype(np.float32)
    mag = rng.exponential(1e-5, M).astype(np.float32)
    nic = np.zeros(N, np.int32)
    nic[:N_VALID] = rng.integers(1, 20, N_VALID)
    acc = dict(accumulated_num_in_camera=nic, accumulated_num_pixels=(nic * rng.integers(0, 1000, N)).astype(np.int32),
               accumulated_view_space_position_gradients=(nic * rng.exponential(1e-5, N)).astype(np.float32),
               accumulated_view_space_position_gradients_avg=(nic * rng.exponential(1e-8, N)).astype(np.float32),
               accumulated_position_gradients=(nic[:, None] * rng.normal(0, 1e-3, (N, 3))).astype(np.float32),
               accumulated_position_gradients_norm=(nic * rng.exponential(1e-3, N)).astype(np.float32))
    alpha = ft[:N_VALID, 7]
    mfn = acc["accumulated_position_gradients_norm"][:N_VALID] / nic[:N_VALID]
    inf = float("inf")
    cfg = Ctl.GaussianPointAdaptiveControllerConfig(
        transparent_alpha_threshold=float(np.quantile(alpha, 0.008)),           # ~0.8 % transparent
        floater_near_camrea_num_pixels_threshold=int(np.quantile(npix, 0.99)),  # ~1 % of the view's points
        floater_depth_threshold=3.0,                                             # ... of which the near eighth: ~0.2 % of the rows
        densification_view_space_position_gradients_threshold=float(np.quantile(mag, 0.975)),   # ~1 % of the valid rows
        densification_view_avg_space_position_gradients_threshold=inf,
        densification_multi_frame_view_space_position_gradients_threshold=inf,
        densification_multi_frame_view_pixel_avg_space_position_gradients_threshold=inf,
        densification_multi_frame_position_gradients_threshold=float(np.quantile(mfn, 0.96)),   # ~4 %
        under_reconstructed_num_pixels_threshold=5000)
    scene = dict(pc=pc, feat=ft, mask=mask, obj=obj)
    hook = dict(ids=ids, npix=npix, depth=depth, mag=mag)
    return scene, acc, hook, cfg


def timed(fn, restore, reps, warmup):
    times = []
    for r in range(reps + warmup):
        restore()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if r >= warmup:
            times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("path", nargs="?", help="where to write the result (same as --out)")
    ap.add_argument("--rows", type=int, default=500_000, help="valid rows (the arrays hold twice as many)")
    ap.add_argument("--in-camera", type=int, default=200_000, help="points of the view's hook")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(H.ROOT, "profiles", "density_bench.json"))
    a = ap.parse_args()
    H.require_gpu("bench_densify.py")
    DEV = torch.device("cuda:0")
    N_VALID, M, REPS = a.rows, a.in_camera, a.steps
    scene, acc, hook, cfg = make_workload(N_VALID, M)
    N = scene["pc"].shape[0]
    orig = {k: torch.tensor(v, device=DEV) for k, v in scene.items()}
    live = {k: v.clone() for k, v in orig.items()}
    acc_d = {k: torch.tensor(v, device=DEV) for k, v in acc.items()}
    hook_d = {k: torch.tensor(v, device=DEV) for k, v in hook.items()}

    def restore():
        for k in live:
            live[k].copy_(orig[k])

    ctl = Ctl(cfg, Ctl.GaussianPointAdaptiveControllerMaintainedParameters(live["pc"], live["feat"], live["mask"], live["obj"]), seed=0)
    for k, v in acc_d.items():
        getattr(ctl.accumulators, k).copy_(v)
    ctl.iteration_counter = cfg.iteration_start_remove_floater + 1
    payload = types.SimpleNamespace(point_id_in_camera_list=hook_d["ids"], num_affected_pixels=hook_d["npix"],
                                    point_depth=hook_d["depth"], magnitude_grad_viewspace=hook_d["mag"])

    def hip_step():
        ctl._find_densify_points(payload)
        ctl._add_densify_points()

    def hip_select():
        ctl._find_densify_points(payload)

    def torch_step():
        info = find_densify_points(live["pc"], live["feat"], live["mask"], acc_d, hook_d["ids"], hook_d["npix"], hook_d["depth"],
                                   hook_d["mag"], True, cfg)
        add_densify_points(live["pc"], live["feat"], live["mask"], live["obj"], info, cfg, 0, 0)

    hip_med, hip_min = timed(hip_step, restore, REPS, a.warmup)
    sel_med, _ = timed(hip_select, restore, REPS, a.warmup)
    counts = ctl.last_refinement_counts()
    torch_med, torch_min = timed(torch_step, restore, REPS, a.warmup)
    res = dict(what="one densification: select + apply (device events, host syncs of the torch path included)",
               n_rows=N, n_valid=N_VALID, n_in_camera=M, reps=REPS, device=torch.cuda.get_device_name(0),
               counts=counts, densify_fraction_of_valid=counts["densify"] / N_VALID,
               pruned_fraction_of_valid=(counts["floaters"] + counts["transparent"]) / N_VALID,
               hip_select_apply_ms_median=hip_med, hip_select_apply_ms_min=hip_min, hip_select_ms_median=sel_med,
               torch_reference_ms_median=torch_med, torch_reference_ms_min=torch_min, speedup_median=torch_med / hip_med)
    H.write_json(res, a.path or a.out, indent=None)


if __name__ == "__main__":
    main()
