#!/usr/bin/env python3
"""Time the mesh path (fusion.py: gs_tsdf_integrate, gs_isosurface_plan, gs_isosurface_emit, include/gs_fusion.h) on cuda:0:
--views (16) frames of --workload (cfg3_headline: 500 000 rows, 1920 x 1088) rendered with depth and accumulated alpha under
synthetic.view_pose(i, views), fused into G^3 volumes over mixture.bounding_box of the scene, G = 256 and 512 (--grids).

Per G:
  integrate     one TSDFVolume.integrate() call with all the views (launches of fusion.VIEWS_PER_LAUNCH views), with and without
                the colour volume: device events around each call after the warm-up (harness.per_call_ms: host side included),
                median / p10 / p90, and the achieved bytes per second against the volume's own traffic -- every voxel's tsdf and
                weight (and colour) read once and written once per launch, 16 (40) bytes; the gathers from the frames are not counted
  isosurface    TSDFVolume.extract_mesh() on the fused volume: plan, the host read of the two totals, the allocations and emit,
                timed as one call the same way; V and F recorded
  torch         the same fusion restated with torch operations on the same device, the whole voxel grid against one view at a
                time (host clock around one pass over the views ending in a synchronise, after one untimed view): what a user
                would write without the kernel.  It is first checked against ours on a fresh volume (the largest absolute
                difference of tsdf is recorded).  A leg whose largest tensor has 2^31 elements or more, or whose working set
                is projected above --baseline-gib, is not started: the record says "not run" and why.

Writes the result (with _native.source_digest()) to --out, default profiles/fusion_bench.json, and prints it."""
import argparse
import os
import sys

import harness as H
import numpy as np
import torch

from taichi_3d_gaussian_splatting_amd import CameraInfo, _native, fusion, mixture
from taichi_3d_gaussian_splatting_amd.synthetic import make_scene, scene_input, view_pose

DEV = "cuda:0"
ELEMENT_LIMIT = 2 ** 31
BASELINE_TEMPORARIES = 24          # G^3 f32 tensors alive at once in the torch leg, counted generously


def render_views(scene, n_views):
    """-> [(depth, alpha, image, q, t)] of the scene under view_pose(i, n_views)"""
    from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast
    module = Rast(Rast.GaussianPointCloudRasterisationConfig(near_plane=0.8, far_plane=1000., depth_to_sort_key_scale=100.))
    out = []
    with torch.no_grad():
        for i in range(n_views):
            q, t = view_pose(i, n_views)
            image, depth, _, alpha = module(scene_input(scene, q, t, DEV), return_accumulated_alpha=True)
            out.append((depth, alpha, image, q[0], t[0]))
    return out


def torch_fusion(tsdf, weight, colour, grid, views, intrinsics, p):
    """the rule of gs_tsdf_integrate with torch operations, the whole grid against one view at a time, in place"""
    px, py, pz = grid
    fx, fy, cx, cy = intrinsics
    for depth, alpha, image, q, t in views:
        m = fusion.world_to_camera(q, t)
        h, w = depth.shape
        x = ((float(m[0, 0]) * px + float(m[0, 1]) * py) + float(m[0, 2]) * pz) + float(m[0, 3])
        y = ((float(m[1, 0]) * px + float(m[1, 1]) * py) + float(m[1, 2]) * pz) + float(m[1, 3])
        z = ((float(m[2, 0]) * px + float(m[2, 1]) * py) + float(m[2, 2]) * pz) + float(m[2, 3])
        u = fx * (x / z) + cx
        v = fy * (y / z) + cy
        keep = (z > p["near"]) & (u >= 0) & (u < w) & (v >= 0) & (v < h)
        zero = torch.zeros_like(u)
        pixel = torch.where(keep, torch.floor(v), zero).to(torch.int64) * w + torch.where(keep, torch.floor(u), zero).to(torch.int64)
        d = depth.reshape(-1)[pixel]
        keep &= (d > 0) & torch.isfinite(d) & (alpha.reshape(-1)[pixel] >= p["min_alpha"])
        sdf = d - z
        keep &= ~(sdf < -p["trunc"])
        s = torch.clamp(sdf / p["trunc"], max=1.0)
        Wn = weight + 1.0
        tsdf.copy_(torch.where(keep, (weight * tsdf + s) / Wn, tsdf))
        if colour is not None:
            rgb = image.reshape(-1, 3)[pixel]
            colour.copy_(torch.where(keep.unsqueeze(-1), (weight.unsqueeze(-1) * colour + rgb) / Wn.unsqueeze(-1), colour))
        weight.copy_(torch.where(keep, torch.clamp(Wn, max=p["max_weight"]), weight))


def baseline_leg(volume, views, camera, intrinsics, a):
    """the torch restatement on a volume of the same shape -> its record"""
    n = volume.tsdf.numel()
    largest = 3 * n                                                    # the colour volume
    need_gib = BASELINE_TEMPORARIES * n * 4 / 2 ** 30
    if largest >= ELEMENT_LIMIT:
        return {"status": "not run", "reason": f"its largest tensor has {largest:.3g} elements; no leg with 2^31 elements or more in one tensor is started"}
    if need_gib > a.baseline_gib:
        return {"status": "not run", "reason": f"its working set is projected at {need_gib:.0f} GiB (limit {a.baseline_gib} GiB)"}
    p = dict(trunc=volume.trunc, max_weight=volume.max_weight, min_alpha=volume.min_alpha, near=volume.near)
    try:
        axes = [torch.arange(volume.dims[k], device=DEV, dtype=torch.float32) * volume.voxel[k] + volume.origin[k] for k in range(3)]
        grid = [g.contiguous() for g in torch.meshgrid(*axes, indexing="ij")]
        state = lambda: (torch.ones_like(volume.tsdf), torch.zeros_like(volume.weight), torch.zeros_like(volume.colour))
        ours = fusion.TSDFVolume(origin=volume.origin, dims=volume.dims, voxel=volume.voxel, device=DEV, **p)
        ours.integrate(*[[v[k] for v in views] for k in (0, 3, 4)], camera, alpha=[v[1] for v in views], image=[v[2] for v in views])
        tsdf, weight, colour = state()
        torch_fusion(tsdf, weight, colour, grid, views, intrinsics, p)
        difference = float((tsdf - ours.tsdf).abs().max())
        differing = float((tsdf != ours.tsdf).float().mean())
        del ours
        tsdf, weight, colour = state()
        torch_fusion(tsdf, weight, colour, grid, views[:1], intrinsics, p)                # untimed: allocator warm-up
        ms = float(H.wall_ms(lambda: torch_fusion(tsdf, weight, colour, grid, views, intrinsics, p), 1, 0))
        return {"status": "run", "all_views_ms": ms, "largest_abs_tsdf_difference_to_ours": difference, "share_of_voxels_differing": differing}
    except torch.cuda.OutOfMemoryError as e:
        torch.cuda.empty_cache()
        return {"status": "not run", "reason": "out of device memory: " + str(e).split("\n")[0][:160]}


def measure_grid(G, bbox, views, camera, intrinsics, a):
    print(f"bench_fusion: G = {G}", file=sys.stderr, flush=True)
    rec = {"voxels": G ** 3, "integrate": {}}
    lists = [[v[k] for v in views] for k in range(5)]
    volume = None
    for name, colour, voxel_bytes in (("without_colour", False, 16), ("with_colour", True, 40)):
        volume = fusion.TSDFVolume(bbox=bbox, dims=G, colour=colour, near=0.8, device=DEV)
        call = lambda: volume.integrate(lists[0], lists[3], lists[4], camera, alpha=lists[1], image=lists[2])
        t = H.summary(H.per_call_ms(call, a.steps, a.warmup))
        launches = -(-len(views) // fusion.VIEWS_PER_LAUNCH)
        volume_bytes = G ** 3 * voxel_bytes * launches
        rec["integrate"][name] = dict(t, launches=launches, volume_bytes_per_call=volume_bytes, bytes_per_second=volume_bytes / (t["ms_median"] * 1e-3))
    rec["voxel"], rec["trunc"] = volume.voxel, volume.trunc
    mesh = volume.extract_mesh()
    rec["isosurface"] = dict(H.summary(H.per_call_ms(volume.extract_mesh, a.steps, a.warmup)), vertices=int(mesh.vertices.shape[0]),
                             faces=int(mesh.faces.shape[0]), share_of_voxels_seen=float((volume.weight > 0).float().mean()))
    del mesh
    torch.cuda.empty_cache()
    rec["torch_one_view_at_a_time"] = baseline_leg(volume, views, camera, intrinsics, a)
    if rec["torch_one_view_at_a_time"]["status"] == "run":
        rec["integrate"]["with_colour"]["speedup_over_torch"] = round(rec["torch_one_view_at_a_time"]["all_views_ms"] / rec["integrate"]["with_colour"]["ms_median"], 1)
    del volume
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(H.ROOT, "profiles", "fusion_bench.json"))
    ap.add_argument("--workload", default="cfg3_headline", help="a name of synthetic.make_scene")
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--grids", type=int, nargs="+", default=[256, 512], help="volume sizes G (G^3 voxels)")
    ap.add_argument("--steps", type=int, default=5, help="timed calls of the integration and of the extraction per volume")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--baseline-gib", type=float, default=96.0, help="the torch leg runs only if its projected working set is within this")
    a = ap.parse_args()
    H.require_gpu("bench_fusion.py")
    scene = make_scene(a.workload)
    views = render_views(scene, a.views)
    K = np.asarray(scene.camera_intrinsics, np.float32)
    intrinsics = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    camera = CameraInfo(torch.tensor(K), scene.height, scene.width, 0)              # on the host: no read-back per view
    tensors = tuple(torch.tensor(x, device=DEV) for x in (scene.point_cloud, scene.point_cloud_features, scene.point_invalid_mask))
    bbox = mixture.bounding_box(tensors).cpu()
    out = {"component": "meshes from a scene: depth frames fused into a G^3 truncated signed distance volume (gs_tsdf_integrate) and the "
                        "marching-tetrahedra isosurface of it (gs_isosurface_plan, gs_isosurface_emit), beside the same fusion written "
                        "with torch operations one view at a time, one GPU (see device)",
           "method": "ours: device events around each call after the warm-up, median / p10 / p90 of the per-call milliseconds; bytes_per_second = "
                     "the volume's own read + write bytes per call / median; torch leg: host clock around one pass over the views ending in "
                     "a synchronise, after one untimed view",
           "source_digest": _native.source_digest(), "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
           "workload": a.workload, "n_rows": int(scene.point_cloud.shape[0]), "views": a.views, "image": [scene.height, scene.width],
           "views_per_launch": fusion.VIEWS_PER_LAUNCH, "bbox": bbox.tolist(), "baseline_limit_gib": a.baseline_gib,
           "grids": {f"G={G}": measure_grid(G, bbox, views, camera, intrinsics, a) for G in a.grids}}
    H.write_json(out, a.out)


if __name__ == "__main__":
    main()
