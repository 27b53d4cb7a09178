#!/usr/bin/env python3
"""Measure the touched-row list and the row-selective Adam step (include/gs_sparse.h) against the dense step on cuda:0, at
cfg3_headline, cfg2_truck7k and cfg3_clustered: the touched share T/M and T/N of one training view, the time of
gs_touched_rows, the two-tensor Adam step (features (N,56) and positions (N,3)) dense against selective, and the whole
training iteration (operator + fused loss + Adam) both ways.

Both trainers run with lr = 0 so that they render the same scene in every window (see Trainer).  Every timed leg is a
window of many calls between two device events, ended by a synchronise; the dense and the selective variant alternate,
REPEATS windows each, and the file reports the median and the spread (min, max) of the per-call times.  All legs run in
this one process.  Kernel times are not taken here: run `rocprofv3 --kernel-trace --stats -- python
tools/bench_sparse_step.py --only-iteration sparse|dense [--workload NAME]` for them, in a run of its own.

Writes the result (with _native.source_digest()) to --out, default profiles/sparse_step_bench.json, and prints it."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from taichi_3d_gaussian_splatting_amd import CameraInfo, GaussianPointCloudRasterisation as Rast, _native, sparse  # noqa: E402
from taichi_3d_gaussian_splatting_amd.LossFunction import LossFunction  # noqa: E402
from taichi_3d_gaussian_splatting_amd.optim import FusedAdam  # noqa: E402
from taichi_3d_gaussian_splatting_amd.synthetic import make_scene, view_pose  # noqa: E402

DEV = torch.device("cuda:0")
WORKLOADS = ("cfg3_headline", "cfg2_truck7k", "cfg3_clustered")
REPEATS = 5
FIXED_GRID = 2048          # GS_ADAM_ROWS_GRID of the "fixed grid that strides to the count" shape of k_adam_rows


def window_ms(fn, n):
    """per-call time of n calls between two device events; the window ends in a synchronise"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def alternate(variants, n, warm):
    """variants {name: fn or (fn, environment for its calls)}, warmed up, then timed in turn REPEATS times
    -> {name: {median_ms, min_ms, max_ms, windows_ms}}"""
    variants = {name: v if isinstance(v, tuple) else (v, {}) for name, v in variants.items()}

    def run(fn, env, count, timed):
        os.environ.update(env)
        try:
            if timed:
                return window_ms(fn, count)
            for _ in range(count):
                fn()
        finally:
            for k in env:
                del os.environ[k]
    for fn, env in variants.values():
        run(fn, env, warm, False)
    torch.cuda.synchronize()
    got = {name: [] for name in variants}
    for _ in range(REPEATS):
        for name, (fn, env) in variants.items():
            got[name].append(run(fn, env, n, True))
    return {name: dict(median_ms=round(statistics.median(v), 5), min_ms=round(min(v), 5), max_ms=round(max(v), 5),
                       windows_ms=[round(x, 5) for x in v], calls_per_window=n) for name, v in got.items()}


class Trainer:
    """One training loop of the workload: operator, fused loss, FusedAdam on features and positions"""

    def __init__(self, s, selective):
        H, W = s.height, s.width
        q, t = view_pose()
        self.pc = torch.tensor(s.point_cloud, device=DEV, requires_grad=True)
        self.feat = torch.tensor(s.point_cloud_features, device=DEV, requires_grad=True)
        self.mask, obj = torch.tensor(s.point_invalid_mask, device=DEV), torch.tensor(s.point_object_id, device=DEV)
        self.rast = Rast(Rast.GaussianPointCloudRasterisationConfig())
        self.rast.track_touched_rows = bool(selective)
        self.selective = bool(selective)
        self.inp = Rast.GaussianPointCloudRasterisationInput(
            point_cloud=self.pc, point_cloud_features=self.feat, point_object_id=obj, point_invalid_mask=self.mask,
            camera_info=CameraInfo(torch.tensor(s.camera_intrinsics, device=DEV), H, W, 0),
            q_pointcloud_camera=torch.tensor(q, device=DEV), t_pointcloud_camera=torch.tensor(t, device=DEV), color_max_sh_band=3)
        self.gt = torch.rand(3, H, W, device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
        # lr = 0: the kernels stream the same bytes and do the same arithmetic at any learning rate, and the dense and the
        # selective trainer keep rendering the SAME scene however many steps each has taken (with a real lr the two scenes
        # drift apart over the windows and the rasteriser's own time with them)
        self.of, self.op = FusedAdam([self.feat], lr=0.0), FusedAdam([self.pc], lr=0.0)
        self.loss_fn = LossFunction(LossFunction.LossFunctionConfig())

    def backward(self):
        self.of.zero_grad(); self.op.zero_grad()
        img, _, _ = self.rast(self.inp)
        L = self.loss_fn(img.permute(2, 0, 1), self.gt, point_invalid_mask=self.mask, pointcloud_features=self.feat, clamp_predicted=True)[0]
        L.backward()

    def step(self):
        rows = self.rast.last_touched_rows if self.selective else None
        self.of.step(rows=rows); self.op.step(rows=rows)

    def iteration(self):
        self.backward()
        self.step()


def measure(name):
    s = make_scene(name)
    N = s.point_cloud.shape[0]
    out = {"n_points": N, "image": [s.width, s.height]}
    sp, de = Trainer(s, True), Trainer(s, False)
    # one view: the share of rows the backward touched
    sp.backward()
    frame, rows = sp.rast.last_frame, sp.rast.last_touched_rows
    T, M = int(rows.count.item()), rows.max_count
    out.update(n_points_in_camera=M, n_touched=T, touched_of_in_camera=round(T / max(M, 1), 4), touched_of_all=round(T / max(N, 1), 4),
               compaction_workgroups=-(-M // sparse.COMPACT_BLOCK))
    # the list alone: the frame's backward stays the context's latest, so the call can be repeated
    out["gs_touched_rows_ms"] = alternate({"gs_touched_rows": lambda: sparse.touched_rows(frame)}, n=200, warm=20)["gs_touched_rows"]
    # the two-tensor Adam step on this view's gradients, dense against selective (both shapes of the selective launch)
    de.backward()
    torch.cuda.synchronize()

    out["adam_two_tensors_ms"] = alternate({"dense": de.step, "selective": sp.step,
                                            f"selective_fixed_grid_{FIXED_GRID}": (sp.step, {"GS_ADAM_ROWS_GRID": str(FIXED_GRID)})},
                                           n=200, warm=20)
    out["adam_two_tensors_ms"]["selective_plus_list_median_ms"] = round(
        out["adam_two_tensors_ms"]["selective"]["median_ms"] + out["gs_touched_rows_ms"]["median_ms"], 5)
    # the whole training iteration both ways
    out["training_iteration_ms"] = alternate({"dense": de.iteration, "selective": sp.iteration}, n=100, warm=20)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_step_bench.json"))
    ap.add_argument("--workload", action="append", choices=WORKLOADS)
    ap.add_argument("--only-iteration", choices=("dense", "sparse"), help="for rocprofv3: nothing but that iteration's launches")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse_step.py needs the GPU: there is nothing to measure without one")
    names = a.workload or list(WORKLOADS)
    if a.only_iteration:
        tr = Trainer(make_scene(names[0]), a.only_iteration == "sparse")
        print(json.dumps({names[0]: {a.only_iteration: alternate({"iteration": tr.iteration}, n=100, warm=20)["iteration"]}}))
        return
    out = {"component": "touched-row list and row-selective Adam step against the dense step, 1x MI355X",
           "method": f"device events around windows of calls ending in a synchronise; variants alternate, {REPEATS} windows each; "
                     "per-call milliseconds; lr = 0 in both trainers (same scene in every window)", "source_digest": _native.source_digest(), "device": torch.cuda.get_device_name(0),
           "workloads": {name: measure(name) for name in names}}
    text = json.dumps(out, indent=1)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
