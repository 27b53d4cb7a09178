"""Start/end time of every k_blend_bwd_tile wave of one backward (stats build): wave durations and how many waves are
resident over the launch, i.e. how much of the launch is tail.  `make -C taichi_3d_gaussian_splatting_amd/csrc times` first (the timing-only diagnostic build: the counting build's
atomics make every wave tens of times slower)."""
import argparse
import ctypes as C
import os

import harness as H
import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="cfg3_headline")
    wl = ap.parse_args().workload
    H.require_gpu("bwd_wave_timeline.py")
    H.use_library("libgsrast_times.so")
    from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast, _native
    from taichi_3d_gaussian_splatting_amd.synthetic import make_scene, scene_input, view_pose
    s = make_scene(wl)
    inp = scene_input(s, *view_pose(), torch.device("cuda", 0), requires_grad=True)
    module = Rast(Rast.GaussianPointCloudRasterisationConfig(), backward_valid_point_hook=lambda p: None)
    for _ in range(3):
        inp.point_cloud.grad = inp.point_cloud_features.grad = None
        image, _, _ = module(inp)
        image.backward(2.0 * (image.detach() - 0.5))
    torch.cuda.synchronize()
    T = ((s.height + 15) // 16) * ((s.width + 15) // 16)
    G = int(os.environ.get("GS_BWD_WAVES_PER_TILE", 0)) or (4 if T < 2000 else 2 if T < 6144 else 1)     # gs_api.hip: waves_per_tile
    n_heavy = module.last_frame.heavy_tiles()
    n_items = module.last_frame.heavy_tiles(items=True)
    # one record per wave, indexed by workgroup * 4 + wave: the heavy tiles' work items first (one workgroup each: a 512-entry segment of
    # a cut list, or a whole list), then the ordinary work items four to a workgroup (k_backward.hip: k_blend_bwd_tile)
    nrec = min(4 * (n_items + ((T - n_heavy) * G + 3) // 4), 65536)
    buf = (C.c_ulonglong * (2 * nrec))()
    _native.lib().gs_debug_wave_times_read(buf, nrec)
    a = np.array(buf, dtype=np.uint64).reshape(nrec, 2).astype(np.int64)
    idx = np.arange(a.shape[0])
    keep = a[:, 1] > a[:, 0]
    a, idx = a[keep], idx[keep]
    keep = a[:, 1] > np.percentile(a[:, 0], 10)
    a, idx = a[keep], idx[keep]        # (a wave that left at once wrote nothing: its slot still holds a stamp of the forward blend, which ended before this launch began)
    T = a.shape[0]
    print(f"{wl}: {n_heavy} heavy tiles handed out as {n_items} work items (4 cooperating waves each), {G} wave(s) per ordinary tile")
    heavy_waves = 4 * n_items
    t0 = a[:, 0].min()
    st, en = (a[:, 0] - t0).astype(float), (a[:, 1] - t0).astype(float)      # wall-clock ticks (only ratios are used)
    dur = en - st
    span = en.max()
    print(f"{wl}: {G} wave(s) per tile; longest wave / launch span = {dur.max() / span:.3f}")
    print(f"{T} waves, launch span {span:.0f} ticks of the 100 MHz wall clock = {span / 100:.1f} us; wave duration mean {dur.mean() / 100:.1f} us, max {dur.max() / 100:.1f}, p99 {np.percentile(dur, 99) / 100:.1f}, min {dur.min() / 100:.1f}")
    print(f"sum of wave durations / (span * 5120 slots) = {dur.sum() / (span * 5120):.3f}")
    for frac in (0.25, 0.5, 0.75, 0.9, 1.0):
        tt = span * frac - 1e-6
        print(f"  at {frac:4.2f} of the span: {int(((st <= tt) & (en > tt)).sum())} waves resident")
    print("first waves (heaviest tiles): durations", np.round(dur[:8], 1), " last:", np.round(dur[-8:], 1))
    late = np.argsort(en)[-5:]
    print("last five waves to finish: block ids", late, "start", np.round(st[late], 1), "dur", np.round(dur[late], 1))
    print("by decile of dispatch order (heaviest first): mean start, mean duration, max end (fractions of the span)")
    for d in range(10):
        sl = slice(d * T // 10, (d + 1) * T // 10)
        print(f"  {d}: start {st[sl].mean() / span:5.2f}  dur {dur[sl].mean() / span:5.2f}  max end {en[sl].max() / span:5.2f}")
    longest = np.argsort(dur)[-8:]
    print("longest waves: block ids", longest, "durations/span", np.round(dur[longest] / span, 2), "start/span", np.round(st[longest] / span, 2))

    hv = idx < heavy_waves
    if hv.any() and (~hv).any():
        print(f"heavy items: {hv.sum()} waves, duration mean {dur[hv].mean() / 100:.1f} us max {dur[hv].max() / 100:.1f}, last end {en[hv].max() / span:.2f} of the span; "
              f"ordinary: {(~hv).sum()} waves, mean {dur[~hv].mean() / 100:.1f} us max {dur[~hv].max() / 100:.1f}, last end {en[~hv].max() / span:.2f}")

    if os.environ.get("GS_TIMELINE_DUMP"):      # raw records for a closer look: wave id, start, end (ticks from the first start), plus the tile lists' lengths
        lens = (module.last_frame.export("tile_points_end").cpu().numpy().astype(np.int64)
                - module.last_frame.export("tile_points_start").cpu().numpy().astype(np.int64))
        np.savez(os.environ["GS_TIMELINE_DUMP"], idx=idx, st=st, en=en, n_heavy=n_heavy, n_items=n_items, G=G, tile_len=lens)


if __name__ == "__main__":
    main()
