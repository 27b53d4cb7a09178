"""Event counters of the two blend kernels on one workload (diagnostic; needs `make -C taichi_3d_gaussian_splatting_amd/csrc stats`).

    GSRAST_LIB=taichi_3d_gaussian_splatting_amd/lib/libgsrast_stats.so python tools/blend_stats.py [workload]

Prints how many 64-entry batches, culled-in entries, evaluated (splat, 8x8 quadrant) pairs and contributing lanes
each kernel went through, next to the per-pixel evaluation count E of the reference algorithm.
"""
import argparse
import ctypes as C
import json

import harness as H
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="cfg3_headline")
    wl = ap.parse_args().workload
    H.require_gpu("blend_stats.py")
    H.use_library("libgsrast_stats.so")
    from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast, _native
    from taichi_3d_gaussian_splatting_amd.synthetic import make_scene, scene_input, view_pose
    dev = torch.device("cuda", 0)
    s = make_scene(wl)
    inp = scene_input(s, *view_pose(), dev, requires_grad=True)
    module = Rast(Rast.GaussianPointCloudRasterisationConfig())
    L = _native.lib()
    buf = (C.c_ulonglong * 32)()
    image, _, _ = module(inp)
    L.gs_debug_stats_read(buf, 1)                 # discard anything earlier
    image, _, _ = module(inp)
    image.backward(2.0 * (image.detach() - 0.5))
    torch.cuda.synchronize()
    L.gs_debug_stats_read(buf, 1)
    c = list(buf)
    fr_last = module.last_forward_outputs["pixel_offset_of_last_effective_point"].to(torch.int64)
    with torch.no_grad():
        module(inp)
    fr = module.last_frame
    tx = (s.width + 15) // 16
    tile_of_pixel = (torch.arange(s.height, device=dev) // 16)[:, None] * tx + (torch.arange(s.width, device=dev) // 16)[None, :]
    E = int((fr_last - fr.export("tile_points_start").to(torch.int64)[tile_of_pixel]).clamp_(min=0).sum().item())
    out = {
        "workload": wl, "sort_pairs": fr.n_keys, "tiles": fr.n_tiles, "pixel_entry_evaluations_E": E,
        "fwd": {"batches_x_waves": c[0], "entries_kept_by_cull": c[1], "quadrant_evals": c[2], "quadrant_evals_rejected_by_exponent": c[4],
                "lanes_contributing": c[3], "lanes_alive": c[5]},
        "bwd": {"batches": c[8], "splat_iterations": c[9], "quadrant_evals_entered": c[10], "quadrant_evals_past_exponent": c[11],
                "quadrant_evals_with_a_contribution": c[15], "lanes_contributing": c[12], "reductions": c[13], "exact_exp_fallbacks": c[14]},
    }
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
