"""Host-side cost of one fwd+bwd step against the GPU time of the same step (diagnostic).

The forward hands M and K to the host once per frame.  With predicted sizing (default) the host reads them AFTER it has queued
the whole forward, so the wait costs the GPU nothing; with GS_PREDICT_SIZES=0 it waits in the middle of the frame with the GPU
idle behind it.  Prints, per step: host time inside forward / loss / backward, the time spent waiting for the counters
(gs_ctx_counter_wait_ns) and how each frame was sized.  Run it once with and once without GS_PREDICT_SIZES=0."""
import argparse
import os
import time

import harness as H
import torch

from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast, _native
from taichi_3d_gaussian_splatting_amd.synthetic import make_scene, scene_input, view_pose


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="cfg3_headline")
    wl = ap.parse_args().workload
    H.require_gpu("host_timeline.py")
    dev = torch.device("cuda", 0)
    inp = scene_input(make_scene(wl), *view_pose(), dev, requires_grad=True)
    module = Rast(Rast.GaussianPointCloudRasterisationConfig(), backward_valid_point_hook=lambda p: None)
    marks = {"fwd": 0.0, "loss": 0.0, "bwd": 0.0}

    def step():
        inp.point_cloud.grad = None
        inp.point_cloud_features.grad = None
        a = time.perf_counter()
        image, _, _ = module(inp)
        b = time.perf_counter()
        g = 2.0 * (image.detach() - 0.5)
        c = time.perf_counter()
        image.backward(g)
        d = time.perf_counter()
        marks["fwd"] += b - a; marks["loss"] += c - b; marks["bwd"] += d - c

    for _ in range(30):
        step()
    torch.cuda.synchronize()
    for k in marks:
        marks[k] = 0.0
    n = 200
    L = _native.lib()
    ctx = module._ctx_for(dev)
    w0 = L.gs_ctx_counter_wait_ns(ctx)
    sizing = {}
    t0 = time.perf_counter()
    for _ in range(n):
        step()
        sizing[module.last_frame.sizing] = sizing.get(module.last_frame.sizing, 0) + 1
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    wait_us = (L.gs_ctx_counter_wait_ns(ctx) - w0) / 1e3 / n
    print(f"GS_PREDICT_SIZES={os.environ.get('GS_PREDICT_SIZES', '1')}: frames sized {sizing}")
    print(f"host loop {1e6 * (t1 - t0) / n:.1f} us/step, with final sync {1e6 * (t2 - t0) / n:.1f} us/step; "
          f"waiting for the frame counters {wait_us:.1f} us/step "
          f"({'after the last launch of the forward: the GPU is busy meanwhile' if os.environ.get('GS_PREDICT_SIZES', '1')[:1] != '0' else 'in the middle of the forward: the GPU has nothing queued behind the per-point kernels'})")
    print("host time inside: " + ", ".join(f"{k} {1e6 * v / n:.1f} us" for k, v in marks.items()) +
          "  (fwd includes waiting for the GPU to publish M and K)")
    # the same with the GPU idle in between (host cost alone: nothing to wait for except the prologue kernels)
    for k in marks:
        marks[k] = 0.0
    for _ in range(50):
        torch.cuda.synchronize()
        step()
    torch.cuda.synchronize()
    print("host time, GPU drained before each step: " + ", ".join(f"{k} {1e6 * v / 50:.1f} us" for k, v in marks.items()))


if __name__ == "__main__":
    main()
