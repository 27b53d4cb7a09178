"""As bwd_wave_timeline.py, for the forward blend (stats build): one record per (tile, quadrant) wave of the last forward."""
import argparse
import ctypes as C

import harness as H
import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="cfg3_headline")
    wl = ap.parse_args().workload
    H.require_gpu("fwd_wave_timeline.py")
    H.use_library("libgsrast_times.so")
    from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast, _native
    from taichi_3d_gaussian_splatting_amd.synthetic import make_scene, scene_input, view_pose
    s = make_scene(wl)
    inp = scene_input(s, *view_pose(), torch.device("cuda", 0))
    module = Rast(Rast.GaussianPointCloudRasterisationConfig())
    with torch.no_grad():
        for _ in range(3):
            module(inp)
    torch.cuda.synchronize()
    T = ((s.height + 15) // 16) * ((s.width + 15) // 16)
    n = min(4 * T, 65536)
    buf = (C.c_ulonglong * (2 * n))()
    _native.lib().gs_debug_wave_times_read(buf, n)
    a = np.array(buf, dtype=np.uint64).reshape(n, 2).astype(np.int64)
    t0 = a[:, 0].min()
    st, en = (a[:, 0] - t0).astype(float), (a[:, 1] - t0).astype(float)
    dur = en - st
    span = en.max()
    slots = 8 * 1024
    print(f"{n} waves, wave duration / span: mean {dur.mean() / span:.3f} max {dur.max() / span:.3f} p99 {np.percentile(dur, 99) / span:.3f}")
    print(f"sum of wave durations / (span * {slots} slots) = {dur.sum() / (span * slots):.3f}")
    for frac in (0.25, 0.5, 0.75, 0.9):
        tt = span * frac
        print(f"  at {frac:4.2f} of the span: {int(((st <= tt) & (en > tt)).sum())} waves resident")


if __name__ == "__main__":
    main()
