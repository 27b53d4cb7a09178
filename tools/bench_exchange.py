#!/usr/bin/env python3
"""Measure the device half of the sparse gradient exchange (include/gs_exchange.h) on cuda:0, at cfg3_headline, cfg2_truck7k
and cfg3_clustered: L = 2, 4, 8 different views are rendered once on this GPU with track_touched_rows, and then timed are
exchange.pack_rows of the L views (each into a tensor of its own, and each straight into its slice of one shared buffer),
exchange.stack_packed of the L separately packed lists (the copy the shared buffer avoids), exchange.merge_rows over them, and what the three replace on the device: L - 1 dense `+=` over the 59*N-float gradient buffer.
Recorded beside the times: the touched rows per view, the union, the bytes a rank contributes to the all-gather -- 240 bytes
times the largest count among the lists, what distributed.sparse_reduce_point_gradients sends after its one host read -- the
bytes of the lists at their host-side bound (L * max_count * 240, what is allocated before any count is known) and the dense
236*N.

The collective itself is NOT measured: the exchange over RCCL needs one GPU per rank.

Every leg is a window of many calls between two device events, ended by a synchronise; the legs alternate, REPEATS windows
each, and the file reports the median and the spread (min, max) of the per-call times (harness.alternate).

Writes the result (with _native.source_digest()) to --out, default profiles/exchange_bench.json, and prints it.
--steps sets the calls per window of every leg (default 100), --warmup the untimed calls (10)."""
import argparse
import os

import harness as H
import torch

from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast, _native, exchange
from taichi_3d_gaussian_splatting_amd.distributed import _flat_base
from taichi_3d_gaussian_splatting_amd.synthetic import SMALL, make_scene, scene_input, view_pose

DEV = "cuda:0"
WORKLOADS = ("cfg3_headline", "cfg2_truck7k", "cfg3_clustered")
VIEWS = (2, 4, 8)
REPEATS = 5


def render_views(s, n_views):
    """n_views forwards and backwards of the scene under different poses -> per view (grad_pointcloud, grad_features, their
    flat 59*N buffer, the TouchedRows of that backward)"""
    rast = Rast(Rast.GaussianPointCloudRasterisationConfig())
    rast.track_touched_rows = True
    gen = torch.Generator(device=DEV).manual_seed(7)
    views = []
    for v in range(n_views):
        q, t = view_pose(v, n_views)
        inp = scene_input(s, q, t, DEV, requires_grad=True)
        img = rast(inp)[0]
        target = torch.rand(img.shape, device=DEV, generator=gen)
        img.backward(2.0 * (img.detach() - target))
        gp, gf = inp.point_cloud.grad, inp.point_cloud_features.grad
        flat = _flat_base(gp, gf)
        views.append((gp, gf, flat if flat is not None else torch.cat([gf.reshape(-1), gp.reshape(-1)]), rast.last_touched_rows))
    torch.cuda.synchronize()
    return views


def measure(name, steps, warm):
    s = make_scene(name)
    N = s.point_cloud.shape[0]
    views = render_views(s, max(VIEWS))
    touched = [int(r.count.item()) for _, _, _, r in views]
    out = {"n_points": N, "image": [s.width, s.height], "bytes_dense": 236 * N,
           "n_points_in_camera_per_view": [r.max_count for _, _, _, r in views], "n_touched_per_view": touched, "lists": {}}
    for L in VIEWS:
        mine = views[:L]
        lists = [exchange.pack_rows(gp, gf, r) for gp, gf, _, r in mine]
        packed, counts = exchange.stack_packed(lists)
        union = int(exchange.merge_rows(packed, counts, N)[2].count.item())
        acc = mine[0][2].clone()

        def dense_adds():
            for _, _, flat, _ in mine[1:]:
                acc.add_(flat)
        shared = torch.empty_like(packed)                                    # one buffer for all lists: no copy before the merge

        def pack_into_shared():
            for l, (gp, gf, _, r) in enumerate(mine):
                exchange.pack_rows(gp, gf, r, out=shared[l])
        legs = H.alternate({"pack_rows_all_views": lambda: [exchange.pack_rows(gp, gf, r) for gp, gf, _, r in mine],
                            "pack_rows_into_one_buffer": pack_into_shared,
                            "stack_packed": lambda: exchange.stack_packed(lists),
                            "merge_rows": lambda: exchange.merge_rows(packed, counts, N),
                            "dense_adds": dense_adds}, n=steps or 100, warm=warm, repeats=REPEATS)
        sparse_ms = sum(legs[k]["median_ms"] for k in ("pack_rows_all_views", "stack_packed", "merge_rows"))
        direct_ms = legs["pack_rows_into_one_buffer"]["median_ms"] + legs["merge_rows"]["median_ms"]
        out["lists"][str(L)] = {
            "union_rows": union, "union_of_all": round(union / max(N, 1), 4), "list_stride": int(packed.shape[1]),
            "bytes_per_rank_at_largest_count": max(touched[:L]) * exchange.ROW_BYTES + 4,
            "bytes_lists_at_bound": L * int(packed.shape[1]) * exchange.ROW_BYTES,
            "dense_adds_count": L - 1, "ms": legs,
            "pack_rows_per_view_median_ms": round(legs["pack_rows_all_views"]["median_ms"] / L, 5),
            "pack_into_one_buffer_merge_median_ms": round(direct_ms, 5),
            "pack_into_one_buffer_merge_over_dense_adds": round(direct_ms / max(legs["dense_adds"]["median_ms"], 1e-9), 3),
            "pack_stack_merge_median_ms": round(sparse_ms, 5),
            "pack_stack_merge_over_dense_adds": round(sparse_ms / max(legs["dense_adds"]["median_ms"], 1e-9), 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(H.ROOT, "profiles", "exchange_bench.json"))
    ap.add_argument("--workload", action="append", choices=WORKLOADS + tuple(SMALL))
    ap.add_argument("--steps", type=int, help="calls per window of every leg")
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    H.require_gpu("bench_exchange.py")
    out = {"component": "packed touched rows and their fixed-order merge against the dense adds they replace, 1x MI355X",
           "method": f"device events around windows of calls ending in a synchronise; legs alternate, {REPEATS} windows each; per-call "
                     "milliseconds; L views rendered on one GPU, lists taken from their backwards",
           "not_measured": "the all-gather itself: the exchange over RCCL needs one GPU per rank",
           "source_digest": _native.source_digest(), "device": torch.cuda.get_device_name(0),
           "workloads": {name: measure(name, a.steps, a.warmup) for name in (a.workload or list(WORKLOADS))}}
    H.write_json(out, a.out)


if __name__ == "__main__":
    main()
