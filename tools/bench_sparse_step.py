#!/usr/bin/env python3
"""Measure the touched-row list and the row-selective Adam step (include/gs_sparse.h) against the dense step on cuda:0, at
cfg3_headline, cfg2_truck7k and cfg3_clustered: the touched share T/M and T/N of one training view, the time of
gs_touched_rows, the two-tensor Adam step (features (N,56) and positions (N,3)) dense against selective, and the whole
training iteration (operator + fused loss + Adam) both ways.

Both trainers run with lr = 0 so that they render the same scene in every window (see Trainer).  Every timed leg is a
window of many calls between two device events, ended by a synchronise; the dense and the selective variant alternate,
REPEATS windows each, and the file reports the median and the spread (min, max) of the per-call times.  All legs run in
this one process (harness.window_ms, harness.alternate).  Kernel times are not taken here: run `rocprofv3 --kernel-trace --stats -- python
tools/bench_sparse_step.py --only-iteration sparse|dense [--workload NAME]` for them, in a run of its own.

Writes the result (with _native.source_digest()) to --out, default profiles/sparse_step_bench.json, and prints it.
--steps sets the calls per window of every leg (default 200, the whole iteration 100), --warmup the untimed calls (20)."""
import argparse
import os

import harness as H
import torch

from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast, _native, sparse
from taichi_3d_gaussian_splatting_amd.LossFunction import LossFunction
from taichi_3d_gaussian_splatting_amd.optim import FusedAdam
from taichi_3d_gaussian_splatting_amd.synthetic import SMALL, make_scene, scene_input, view_pose

DEV = "cuda:0"
WORKLOADS = ("cfg3_headline", "cfg2_truck7k", "cfg3_clustered")
REPEATS = 5
FIXED_GRID = 2048          # GS_ADAM_ROWS_GRID of the "fixed grid that strides to the count" shape of k_adam_rows


class Trainer:
    """One training loop of the workload: operator, fused loss, FusedAdam on features and positions"""

    def __init__(self, s, selective):
        q, t = view_pose()
        self.inp = scene_input(s, q, t, DEV, requires_grad=True)
        self.pc, self.feat, self.mask = self.inp.point_cloud, self.inp.point_cloud_features, self.inp.point_invalid_mask
        self.rast = Rast(Rast.GaussianPointCloudRasterisationConfig())
        self.rast.track_touched_rows = bool(selective)
        self.selective = bool(selective)
        self.gt = torch.rand(3, s.height, s.width, device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
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


def measure(name, steps, warm):
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
    out["gs_touched_rows_ms"] = H.alternate({"gs_touched_rows": lambda: sparse.touched_rows(frame)}, n=steps or 200, warm=warm,
                                            repeats=REPEATS)["gs_touched_rows"]
    # the two-tensor Adam step on this view's gradients, dense against selective (both shapes of the selective launch)
    de.backward()
    torch.cuda.synchronize()

    out["adam_two_tensors_ms"] = H.alternate({"dense": de.step, "selective": sp.step,
                                              f"selective_fixed_grid_{FIXED_GRID}": (sp.step, {"GS_ADAM_ROWS_GRID": str(FIXED_GRID)})},
                                             n=steps or 200, warm=warm, repeats=REPEATS)
    out["adam_two_tensors_ms"]["selective_plus_list_median_ms"] = round(
        out["adam_two_tensors_ms"]["selective"]["median_ms"] + out["gs_touched_rows_ms"]["median_ms"], 5)
    # the whole training iteration both ways
    out["training_iteration_ms"] = H.alternate({"dense": de.iteration, "selective": sp.iteration}, n=steps or 100, warm=warm,
                                               repeats=REPEATS)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(H.ROOT, "profiles", "sparse_step_bench.json"))
    ap.add_argument("--workload", action="append", choices=WORKLOADS + tuple(SMALL))
    ap.add_argument("--steps", type=int, help="calls per window of every leg")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only-iteration", choices=("dense", "sparse"), help="for rocprofv3: nothing but that iteration's launches")
    a = ap.parse_args()
    H.require_gpu("bench_sparse_step.py")
    names = a.workload or list(WORKLOADS)
    if a.only_iteration:
        tr = Trainer(make_scene(names[0]), a.only_iteration == "sparse")
        res = H.alternate({"iteration": tr.iteration}, n=a.steps or 100, warm=a.warmup, repeats=REPEATS)["iteration"]
        H.write_json({names[0]: {a.only_iteration: res}}, None)
        return
    out = {"component": "touched-row list and row-selective Adam step against the dense step, 1x MI355X",
           "method": f"device events around windows of calls ending in a synchronise; variants alternate, {REPEATS} windows each; "
                     "per-call milliseconds; lr = 0 in both trainers (same scene in every window)", "source_digest": _native.source_digest(), "device": torch.cuda.get_device_name(0),
           "workloads": {name: measure(name, a.steps, a.warmup) for name in names}}
    H.write_json(out, a.out)


if __name__ == "__main__":
    main()
