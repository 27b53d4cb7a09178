"""Cost of render_channels (gs_channels_forward / gs_channels_backward) on a kept frame, beside the only way to get the same
result without it and beside one walk of the frame:

  new      render_channels forward, and its backward, for C = 3, 16, 64
  staged   ceil(C / 3) passes of gs_forward_projected + gs_backward_projected over the frame's records with r g b replaced by
           three of the channels (every pass bins, sorts and blends again); d colour of the per-splat sums is the gradient
  walk     k_blend_fwd of the same frame (the library's own kernel timer): the cost of one walk of the lists

Device events around each call (harness.per_call_ms), `--warmup` untimed and `--steps` timed iterations, the two paths
alternating inside one process; the spread quoted is p90 - p10 of the per-iteration times.  The two paths' results are
compared once before timing.
Writes profiles/channels_bench.json (or --out).

    python tools/bench_channels.py [--steps 200] [--warmup 50] [--configs cfg2_truck7k,cfg3_headline] [--channels 3,16,64]
"""
import argparse
import os

import harness as H
import numpy as np
import torch

from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast
from taichi_3d_gaussian_splatting_amd.stages import StagedRasteriser
from taichi_3d_gaussian_splatting_amd.synthetic import make_scene, scene_input, view_pose


def bench_config(name, channels, steps, warmup, dev):
    s = make_scene(name)
    q, t = view_pose()
    N = s.point_cloud.shape[0]
    inp = scene_input(s, q, t, dev)
    cam = inp.camera_info
    module = Rast(Rast.GaussianPointCloudRasterisationConfig())
    walk_ms = H.library_kernel_ms(module, dev, "k_blend_fwd", lambda: module(inp, keep_frame=True), warm=5, reps=50)
    module(inp, keep_frame=True)
    frame = module.last_frame
    ids = frame.export("point_id_in_camera_list").long()
    records = frame.export("records")
    staged = StagedRasteriser(Rast.GaussianPointCloudRasterisationConfig())
    rng = np.random.default_rng(0)
    res = {"n_points": N, "n_points_in_camera": int(frame.n_points_in_camera), "n_keys": int(frame.n_keys), "height": s.height,
           "width": s.width, "k_blend_fwd_ms": walk_ms, "channels": {}}
    for C_ in channels:
        v = torch.tensor(rng.normal(0, 1, (N, C_)).astype(np.float32), device=dev, requires_grad=True)
        G = torch.tensor(rng.normal(0, 1, (s.height, s.width, C_)).astype(np.float32), device=dev)
        passes = (C_ + 2) // 3
        vpad = torch.zeros(N, 3 * passes, device=dev)
        vpad[:, :C_] = v.detach()
        Gpad = torch.zeros(s.height, s.width, 3 * passes, device=dev)
        Gpad[..., :C_] = G
        state = {}

        def new_fwd():
            state["out"] = module.render_channels(v, frame)

        def new_bwd():
            v.grad = None
            state["out"].backward(G, retain_graph=True)

        def old_fwd():
            outs = []
            for k in range(passes):
                rec = records.clone()
                rec[:, 8:11] = vpad[ids, 3 * k:3 * k + 3]
                outs.append(staged.forward_projected(rec, cam, keep=True))
            state["staged"] = outs

        def old_bwd():
            grads = []
            for k, (o, fr) in enumerate(state["staged"]):
                sums, _ = staged.backward_projected(fr, o, Gpad[..., 3 * k:3 * k + 3])
                grads.append(sums[:, 5:8])
            state["staged_grad"] = torch.cat(grads, dim=1)

        # the two paths compute the same thing
        new_fwd(); new_bwd(); old_fwd(); old_bwd()
        image_old = torch.cat([o.rasterized_image for o, _ in state["staged"]], dim=2)[..., :C_]
        out = state["out"].detach()
        fwd_diff = float((out - image_old).abs().max() / out.abs().max())
        grad_new = v.grad[ids]
        grad_diff = float((grad_new - state["staged_grad"][:, :C_]).abs().max() / grad_new.abs().max())
        # alternate the paths: interleaved blocks of a quarter of the steps each
        acc = {k: [] for k in ("new_fwd", "new_bwd", "old_fwd", "old_bwd")}
        block = max(steps // 4, 1)
        for i in range(0, steps, block):
            n = min(block, steps - i)
            w = warmup if i == 0 else 3
            acc["new_fwd"].append(H.per_call_ms(new_fwd, n, w))
            acc["new_bwd"].append(H.per_call_ms(new_bwd, n, w))
            acc["old_fwd"].append(H.per_call_ms(old_fwd, n, w))
            acc["old_bwd"].append(H.per_call_ms(old_bwd, n, w))
        r = {k: H.summary(np.concatenate(x)) for k, x in acc.items()}
        new_ms = r["new_fwd"]["ms_median"] + r["new_bwd"]["ms_median"]
        old_ms = r["old_fwd"]["ms_median"] + r["old_bwd"]["ms_median"]
        spread = max(x["spread_ms"] for x in r.values())
        chunk = 4 if C_ <= 4 else (16 if C_ <= 16 else 32)
        r.update(passes_staged=passes, channel_chunk=chunk, chunks=(C_ + chunk - 1) // chunk,
                 new_fwd_plus_bwd_ms=new_ms, staged_fwd_plus_bwd_ms=old_ms, speedup=old_ms / new_ms, largest_spread_ms=spread,
                 faster_by_more_than_the_spread=bool(old_ms - new_ms > spread),
                 forward_walks_per_chunk=r["new_fwd"]["ms_median"] / ((C_ + chunk - 1) // chunk) / walk_ms,
                 backward_walks_per_chunk=r["new_bwd"]["ms_median"] / ((C_ + chunk - 1) // chunk) / walk_ms,
                 forward_max_diff_to_staged=fwd_diff, backward_max_diff_to_staged=grad_diff)
        res["channels"][str(C_)] = r
        state.clear()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--configs", default="cfg2_truck7k,cfg3_headline")
    ap.add_argument("--channels", default="3,16,64")
    ap.add_argument("--out", default=os.path.join(H.ROOT, "profiles", "channels_bench.json"))
    a = ap.parse_args()
    H.require_gpu("bench_channels.py")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
           "timing": "device events around each call; times include the host side of the calls", "configs": {}}
    for name in a.configs.split(","):
        res["configs"][name] = bench_config(name, [int(c) for c in a.channels.split(",")], a.steps, a.warmup, dev)
    H.write_json(res, a.out)


if __name__ == "__main__":
    main()
