"""Cost of render_channels (gs_channels_forward / gs_channels_backward) on a kept frame, beside the only way to get the same
result without it and beside one walk of the frame:

  new      render_channels forward, and its backward, for C = 3, 16, 64
  staged   ceil(C / 3) passes of gs_forward_projected + gs_backward_projected over the frame's records with r g b replaced by
           three of the channels (every pass bins, sorts and blends again); d colour of the per-splat sums is the gradient
  walk     k_blend_fwd of the same frame (the library's own kernel timer): the cost of one walk of the lists

Device events around each call, `--warmup` untimed and `--steps` timed iterations, the two paths alternating inside one
process; the spread quoted is p90 - p10 of the per-iteration times.  The two paths' results are compared once before timing.
Writes profiles/channels_bench.json (or --out).

    python tools/bench_channels.py [--steps 200] [--warmup 50] [--configs cfg2_truck7k,cfg3_headline] [--channels 3,16,64]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from taichi_3d_gaussian_splatting_amd import CameraInfo, GaussianPointCloudRasterisation as Rast, _native   # noqa: E402
from taichi_3d_gaussian_splatting_amd.stages import StagedRasteriser                                        # noqa: E402
from taichi_3d_gaussian_splatting_amd.synthetic import make_scene, view_pose                                # noqa: E402


def timed(fn, steps, warmup):
    """-> per-iteration milliseconds of fn() (device events)"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) for a, b in ev])


def stats(ms):
    return dict(ms_median=float(np.median(ms)), ms_p10=float(np.percentile(ms, 10)), ms_p90=float(np.percentile(ms, 90)),
                spread_ms=float(np.percentile(ms, 90) - np.percentile(ms, 10)), steps=int(len(ms)))


def blend_fwd_ms(module, inp, dev, reps):
    """k_blend_fwd of the frame, by the library's kernel timer"""
    L = _native.lib()
    names = L.gs_kernel_names().decode().split(",")
    kid = names.index("k_blend_fwd")
    ctx = module._ctx_for(dev)
    for _ in range(5):
        module(inp, keep_frame=True)
    torch.cuda.synchronize()
    _native.check(L.gs_profile_enable(ctx, C.c_uint64(1 << kid)), "gs_profile_enable")
    for _ in range(reps):
        module(inp, keep_frame=True)
    torch.cuda.synchronize()
    ms, cnt = (C.c_double * len(names))(), (C.c_int64 * len(names))()
    _native.check(L.gs_profile_read(ctx, ms, cnt, len(names), 1), "gs_profile_read")
    _native.check(L.gs_profile_enable(ctx, C.c_uint64(0)), "gs_profile_enable")
    return ms[kid] / max(cnt[kid], 1)


def bench_config(name, channels, steps, warmup, dev):
    s = make_scene(name)
    q, t = view_pose()
    N = s.point_cloud.shape[0]
    cam = CameraInfo(camera_intrinsics=torch.tensor(s.camera_intrinsics, device=dev), camera_height=s.height, camera_width=s.width,
                     camera_id=0)
    inp = Rast.GaussianPointCloudRasterisationInput(
        point_cloud=torch.tensor(s.point_cloud, device=dev), point_cloud_features=torch.tensor(s.point_cloud_features, device=dev),
        point_object_id=torch.tensor(s.point_object_id, device=dev), point_invalid_mask=torch.tensor(s.point_invalid_mask, device=dev),
        camera_info=cam, q_pointcloud_camera=torch.tensor(q, device=dev), t_pointcloud_camera=torch.tensor(t, device=dev),
        color_max_sh_band=3)
    module = Rast(Rast.GaussianPointCloudRasterisationConfig())
    walk_ms = blend_fwd_ms(module, inp, dev, 50)
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
            acc["new_fwd"].append(timed(new_fwd, n, w))
            acc["new_bwd"].append(timed(new_bwd, n, w))
            acc["old_fwd"].append(timed(old_fwd, n, w))
            acc["old_bwd"].append(timed(old_bwd, n, w))
        r = {k: stats(np.concatenate(x)) for k, x in acc.items()}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "channels_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_channels.py needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
           "timing": "device events around each call; times include the host side of the calls", "configs": {}}
    for name in a.configs.split(","):
        res["configs"][name] = bench_config(name, [int(c) for c in a.channels.split(",")], a.steps, a.warmup, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
