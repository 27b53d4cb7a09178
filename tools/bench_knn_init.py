#!/usr/bin/env python3
"""Time the exact 3-nearest-neighbour query behind GaussianPointCloudScene.initialize() (gs_knn, include/gs_knn.h) on cuda:0
and put the reference's own call beside it (GaussianPointCloudScene.py:80-85: a host copy of the cloud, then scipy's
cKDTree(x).query(x, k=4), float64, one thread), on four clouds:

  uniform_1e5, uniform_1e6        uniform in a cube
  clustered_5e5                   the positions of synthetic.synth_clustered's 500 000-point scene (cfg3_clustered)
  clustered_5e5_outliers          the same plus 16 points at 1e4 times its extent: the bounding box grows by four decades

The device time is a device-event pair around each knn.nearest_neighbours(x, 3) call (harness.per_call_ms: host side and the
output allocation included) after --warmup untimed calls; --steps calls, median / p10 / p90.  The host legs are wall-clock
and run once each (they take seconds): the copy the reference pays, the tree and query as written, and the same query with
workers=16.  Where scipy cannot be imported those legs are null and the document says so.  --points N replaces the four
clouds by one uniform cloud of N points and the same with 16 outliers (a rehearsal of the plumbing).

Writes the result (with _native.source_digest()) to --out, default profiles/knn_init_bench.json, and prints it."""
import argparse
import os
import time

import harness as H
import numpy as np
import torch

from taichi_3d_gaussian_splatting_amd import _native, knn
from taichi_3d_gaussian_splatting_amd.synthetic import make_scene

DEV = "cuda:0"
K = 3


def uniform(n):
    return np.random.default_rng(0).uniform(-1.0, 1.0, (int(n), 3)).astype(np.float32)


def with_outliers(x, count=16, factor=1e4):
    rng = np.random.default_rng(1)
    extent = float((x.max(axis=0) - x.min(axis=0)).max())
    d = rng.normal(size=(count, 3))
    far = x.mean(axis=0) + d / np.linalg.norm(d, axis=1, keepdims=True) * extent * factor
    return np.concatenate([x, far.astype(np.float32)])


def clouds(points):
    if points:
        u = uniform(points)
        return {f"uniform_{points}": u, f"uniform_{points}_outliers": with_outliers(u)}
    clustered = np.ascontiguousarray(make_scene("cfg3_clustered").point_cloud, dtype=np.float32)
    return {"uniform_1e5": uniform(1e5), "uniform_1e6": uniform(1e6), "clustered_5e5": clustered,
            "clustered_5e5_outliers": with_outliers(clustered)}


def host_legs(x_dev):
    """wall-clock milliseconds of what the reference does for the same cloud, or None without scipy"""
    t0 = time.perf_counter()
    x = x_dev.detach().cpu().numpy()
    copy_ms = (time.perf_counter() - t0) * 1e3
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return dict(host_copy_ms=copy_ms, ckdtree_query_ms=None, ckdtree_query_workers16_ms=None), None
    t0 = time.perf_counter()
    dist, _ = cKDTree(x).query(x, k=K + 1)
    as_written = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    cKDTree(x).query(x, k=K + 1, workers=16)
    workers = (time.perf_counter() - t0) * 1e3
    return dict(host_copy_ms=copy_ms, ckdtree_query_ms=as_written, ckdtree_query_workers16_ms=workers), dist[:, 1:].mean(axis=1)


def measure(x, steps, warm):
    x_dev = torch.from_numpy(x).to(DEV)
    out = {"n_points": int(x.shape[0]), "extent": float((x.max(axis=0) - x.min(axis=0)).max())}
    out["gs_knn"] = H.summary(H.per_call_ms(lambda: knn.nearest_neighbours(x_dev, K), steps, warm))
    legs, want = host_legs(x_dev)
    out["reference"] = legs
    if want is not None:
        got = knn.mean_neighbour_distance(x_dev, K).cpu().numpy().astype(np.float64)
        nz = want > 0
        out["mean_distance_max_relative_difference"] = float((np.abs(got[nz] - want[nz]) / want[nz]).max())
        ms = out["gs_knn"]["ms_median"]
        out["speedup_over_reference_as_written"] = round((legs["host_copy_ms"] + legs["ckdtree_query_ms"]) / ms, 2)
        out["speedup_over_reference_workers16"] = round((legs["host_copy_ms"] + legs["ckdtree_query_workers16_ms"]) / ms, 2)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(H.ROOT, "profiles", "knn_init_bench.json"))
    ap.add_argument("--points", type=int, help="one uniform cloud of this many points (and the same with 16 outliers) instead of the four")
    ap.add_argument("--steps", type=int, default=20, help="timed calls of gs_knn per cloud")
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    H.require_gpu("bench_knn_init.py")
    try:
        import scipy
        scipy_note = f"scipy {scipy.__version__}"
    except ImportError:
        scipy_note = "scipy is not importable here: the reference's legs are null"
    out = {"component": f"exact {K}-nearest-neighbour query of the scene initialiser (gs_knn) against the reference's cKDTree call, one GPU (see device)",
           "method": "gs_knn: device events around each call after the warm-up, median / p10 / p90 of the per-call milliseconds; reference: "
                     "wall clock, one run each of the host copy, cKDTree(x).query(x, k=4) and the same with workers=16; speedups compare "
                     "copy + query with the gs_knn median", "reference_library": scipy_note, "host_cpus_used": 16,
           "source_digest": _native.source_digest(), "device": torch.cuda.get_device_name(0), "k": K,
           "clouds": {name: measure(x, a.steps, a.warmup) for name, x in clouds(a.points).items()}}
    H.write_json(out, a.out)


if __name__ == "__main__":
    main()
