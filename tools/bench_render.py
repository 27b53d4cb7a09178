#!/usr/bin/env python3
"""Measure how rendered frames leave the device, and the bake, on cuda:0.  A synthetic config-5 scene (2e6 points, sigma0 0.01)
is rendered by the rasteriser's rgb_only path under a few poses at 976x544 and at 1920x1088, in frames per second over at least
200 frames after a warm-up, by a host clock around the whole loop (it ends when the last frame is on the host, or in its file):
  (a) the reference's way: torch.clamp(image * 255, 0, 255).byte().cpu().numpy() per frame (gaussian_point_render.py:121);
  (b) frames.FrameSink with no file written;
  (c) the sink writing ppm to a temporary directory;
  (d) the sink writing png there;
and beside them the render alone, the pieces of a frame's way out on their own (the conversion call against torch's three
kernels, the pinned copy of the bytes against the pageable copy of the f32 frame) and the D2H bandwidth that (b) implies --
a lower bound: the loop also renders.  Last, gs_scene_bake on 5e5 rows against its restatement in torch f32 on the device.
No ratio is asserted.

    python tools/bench_render.py [--out profiles/render_bench.json] [--steps N] [--warmup N] [--points N] [--bake-rows N]
"""
import argparse
import dataclasses
import shutil
import tempfile
import time

import harness as H
import numpy as np
import torch

from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast, compose, frames
from taichi_3d_gaussian_splatting_amd.synthetic import CONFIGS, scene_input, synth, view_pose

DEV = "cuda:0"
RESOLUTIONS = ((544, 976), (1088, 1920))
N_POSES = 8


def torch_bake(pc, ft, q, t, scale, sh):
    """the bake restated with torch f32 ops on the device: what a caller without the kernel would write"""
    R = torch.tensor(compose.quaternion_to_matrix(q), dtype=torch.float32, device=pc.device)
    out_pc = pc @ (scale * R).T + torch.tensor(t, dtype=torch.float32, device=pc.device)
    out = ft.clone()
    b = ft[:, 0:4] / ft[:, 0:4].norm(dim=1, keepdim=True)
    a = torch.tensor(q, dtype=torch.float32, device=pc.device).expand_as(b)
    av, aw, bv, bw = a[:, :3], a[:, 3:4], b[:, :3], b[:, 3:4]
    out[:, 0:4] = torch.cat([aw * bv + bw * av + torch.cross(av, bv, dim=-1), aw * bw - (av * bv).sum(-1, keepdim=True)], dim=-1)
    out[:, 4:7] = ft[:, 4:7] + float(np.log(scale))
    offset = 0
    for lo, hi in compose.BANDS:
        d = hi - lo
        M = torch.tensor(sh[offset:offset + d * d].reshape(d, d), dtype=torch.float32, device=pc.device)
        offset += d * d
        for c in range(3):
            out[:, 8 + 16 * c + lo:8 + 16 * c + hi] = ft[:, 8 + 16 * c + lo:8 + 16 * c + hi] @ M.T
    return out_pc, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--steps", type=int, default=200, help="timed frames of every leg")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--points", type=int, default=CONFIGS["cfg5_infer2e6"]["N"])
    ap.add_argument("--bake-rows", type=int, default=500_000)
    a = ap.parse_args()
    H.require_gpu("bench_render.py")
    module = Rast(Rast.GaussianPointCloudRasterisationConfig(near_plane=0.8, far_plane=1000., depth_to_sort_key_scale=100., rgb_only=True))
    poses = [tuple(torch.tensor(x, device=DEV) for x in view_pose(i, N_POSES)) for i in range(N_POSES)]
    out = {"component": "frames out of the device and the bake, 1x MI355X",
           "scene": {"points": a.points, "sigma0": CONFIGS["cfg5_infer2e6"]["sigma0"], "poses": N_POSES},
           "frames_per_leg": a.steps, "sink_slots": 4, "resolutions": {}}

    for height, width in RESOLUTIONS:
        s = synth(a.points, width, height, CONFIGS["cfg5_infer2e6"]["sigma0"], sh_deg=3, seed=0)
        first = scene_input(s, *view_pose(0, N_POSES), DEV)             # the scene on the device once; the poses take turns
        inputs = [dataclasses.replace(first, q_pointcloud_camera=q, t_pointcloud_camera=t) for q, t in poses]

        def render(i):
            with torch.no_grad():
                return module(inputs[i % N_POSES])[0]

        def fps(frame, finish=lambda: None):
            for i in range(a.warmup):
                frame(i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.steps):
                frame(i)
            finish()
            torch.cuda.synchronize()
            return round(a.steps / (time.perf_counter() - t0), 2)

        def sink_fps(directory, fmt):
            sink = frames.FrameSink(directory, fmt=fmt, slots=4, device=DEV)
            got = fps(lambda i: sink.submit(render(i)), sink.close)
            return got, sink.n_threads

        legs = {"render_only_fps": fps(render),
                "a_reference_clamp_byte_cpu_fps": fps(lambda i: torch.clamp(render(i) * 255, 0, 255).byte().cpu().numpy())}
        legs["b_sink_no_file_fps"], threads = sink_fps(None, "npy")
        tmp = tempfile.mkdtemp(prefix="bench_render_")
        try:
            legs["c_sink_ppm_fps"], _ = sink_fps(tmp, "ppm")
            legs["d_sink_png_fps"], _ = sink_fps(tmp, "png")
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        out["writer_threads"] = threads
        # the pieces on their own
        image = render(0)
        u8 = frames.frame_to_u8(image)
        pinned = torch.empty(u8.shape, dtype=torch.uint8).pin_memory()
        n, warm = max(a.steps, 2), max(min(a.warmup, 10), 1)           # per-call times: a host clock around n calls and a synchronise
        legs["frame_bytes_f32"], legs["frame_bytes_u8"] = image.numel() * 4, u8.numel()
        legs["to_u8_call_ms"] = round(H.wall_ms(lambda: frames.frame_to_u8(image, out=u8), 10 * n, warm), 4)
        legs["torch_clamp_mul_byte_call_ms"] = round(H.wall_ms(lambda: torch.clamp(image * 255, 0, 255).byte(), 10 * n, warm), 4)
        legs["u8_pinned_copy_ms"] = round(H.wall_ms(lambda: pinned.copy_(u8, non_blocking=True), 5 * n, warm), 4)
        legs["f32_pageable_copy_ms"] = round(H.wall_ms(lambda: image.cpu(), 5 * n, warm), 4)
        legs["u8_pinned_copy_gb_per_s"] = round(u8.numel() / legs["u8_pinned_copy_ms"] / 1e6, 2)
        legs["f32_pageable_copy_gb_per_s"] = round(image.numel() * 4 / legs["f32_pageable_copy_ms"] / 1e6, 2)
        legs["d2h_gb_per_s_implied_by_b"] = round(u8.numel() * legs["b_sink_no_file_fps"] / 1e9, 3)
        out["resolutions"][f"{width}x{height}"] = legs
        del first, inputs

    # the bake
    rows = a.bake_rows
    rng = np.random.default_rng(1)
    pc = torch.tensor(rng.normal(0, 2.0, (rows, 3)).astype(np.float32), device=DEV)
    ft = torch.tensor(rng.normal(0, 0.5, (rows, 56)).astype(np.float32), device=DEV)
    q = np.array([0.3, -0.5, 0.1, 0.8]) / np.linalg.norm([0.3, -0.5, 0.1, 0.8])
    t, scale = np.array([0.5, -1.0, 2.0]), 2.5
    sh = compose.sh_rotation_matrices(compose.quaternion_to_matrix(q))
    out_pc, out_ft = torch.empty_like(pc), torch.empty_like(ft)
    n, warm = max(5 * a.steps, 2), max(min(a.warmup, 10), 1)
    got = compose.scene_bake(pc, ft, q, t, scale, out_pc, out_ft)
    want = torch_bake(pc, ft, q, t, scale, sh)
    out["bake"] = {"rows": rows,
                   "call_ms": round(H.wall_ms(lambda: compose.scene_bake(pc, ft, q, t, scale, out_pc, out_ft), n, warm), 4),
                   "torch_f32_on_device_ms": round(H.wall_ms(lambda: torch_bake(pc, ft, q, t, scale, sh), n, warm), 4),
                   "max_abs_difference": float(max((got[0] - want[0]).abs().max(), (got[1] - want[1]).abs().max()))}
    out["bake"]["call_gb_per_s"] = round(rows * 59 * 4 * 2 / out["bake"]["call_ms"] / 1e6, 1)       # rows read and written once
    H.write_json(out, a.out)


if __name__ == "__main__":
    main()
