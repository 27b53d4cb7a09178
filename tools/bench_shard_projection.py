"""Owner side of the Gaussian-parallel scheme on ONE GPU: a shard of N/W Gaussians projected for W views, once with a host
wait per view (gs_project_shard) and once begun back to back and read afterwards (gs_project_shard_begin): milliseconds per
step of that stage alone, GPU otherwise idle, by a host clock around the loop (harness.wall_ms).

    python tools/bench_shard_projection.py [W] [--workload cfg3_headline] [--steps 200] [--warmup 20] [--out PATH]   (GPU)
"""
import argparse
import dataclasses

import harness as H
import torch

from taichi_3d_gaussian_splatting_amd.stages import StagedRasteriser
from taichi_3d_gaussian_splatting_amd.synthetic import make_scene, scene_input, view_pose


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("views", nargs="?", type=int, default=8, help="W: views per step, and the shard is 1/W of the scene")
    ap.add_argument("--workload", default="cfg3_headline")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", help="also write the line there")
    a = ap.parse_args()
    H.require_gpu("bench_shard_projection.py")
    W = a.views
    dev = torch.device("cuda", 0)
    s = make_scene(a.workload)
    n = s.point_cloud.shape[0] // W
    shard = dataclasses.replace(s, point_cloud=s.point_cloud[:n], point_cloud_features=s.point_cloud_features[:n],
                                point_object_id=s.point_object_id[:n], point_invalid_mask=s.point_invalid_mask[:n])
    inputs = [scene_input(shard, *view_pose(v, W), dev) for v in range(W)]
    st = StagedRasteriser()

    def waiting():
        return [st.project_shard(i)[0] for i in inputs]

    def begun():
        frames = [st.project_shard_begin(i) for i in inputs]
        return [st.project_shard_finish(f, want_ids=False)[0] for f in frames]

    out = {"workload": f"{a.workload} shard of {n} Gaussians (1/{W}) projected for {W} views", "steps": a.steps}
    for name, fn in (("wait_per_view_ms", waiting), ("begun_back_to_back_ms", begun)):
        out[name] = round(H.wall_ms(fn, a.steps, a.warmup), 4)
    H.write_json(out, a.out, indent=None)


if __name__ == "__main__":
    main()
