"""Compress a trained scene: python gaussian_point_compress.py IN.parquet OUT.npz [--codes 4096 --iters 10 --seed 0 --poses FILE]

The 45 higher-band SH coefficients of every Gaussian go behind a codebook found by k-means on the GPU, everything else but the
positions to half precision (taichi_3d_gaussian_splatting_amd/compression.py describes the file).  OUT.npz is read by
gaussian_point_render.py --parquet_path, GaussianPointRenderer, SceneComposition and GaussianPointCloudScene.from_compressed.

--poses is a .pt file saved with torch.save() holding (F,4,4) T_pointcloud_camera matrices, or a dataset JSON of the trainer, as
gaussian_point_render.py reads them.  With it every Gaussian is weighted by its share of the pictures from those poses (the
summed blend weight, compression.visibility_weights), and the original and the decoded scene are rendered under every pose:
the PSNR of decoded against original per view is printed.  --image_height / --image_width / --camera_intrinsics fx fy cx cy
replace the renderer's defaults used with a .pt.  One JSON line is printed.
"""
import argparse
import json
import os

import torch

from taichi_3d_gaussian_splatting_amd import compression
from taichi_3d_gaussian_splatting_amd.Camera import CameraInfo
from taichi_3d_gaussian_splatting_amd.GaussianPointCloudRasterisation import GaussianPointCloudRasterisation as Rast
from taichi_3d_gaussian_splatting_amd.GaussianPointCloudScene import GaussianPointCloudScene
from taichi_3d_gaussian_splatting_amd.utils import SE3_to_quaternion_and_translation_torch


def load_poses(path, device, height, width, intrinsics):
    """-> (q (F,4), t (F,3), [CameraInfo per view])"""
    if path.endswith(".pt"):
        q, t = SE3_to_quaternion_and_translation_torch(torch.load(path).to(device=device, dtype=torch.float32))
        info = CameraInfo(camera_intrinsics=intrinsics.to(device=device, dtype=torch.float32), camera_height=height - height % 16,
                          camera_width=width - width % 16, camera_id=0)
        return q, t, [info] * q.shape[0]
    if path.endswith(".json"):
        from taichi_3d_gaussian_splatting_amd.ImagePoseDataset import ImagePoseDataset
        from taichi_3d_gaussian_splatting_amd.targets import TargetStore
        targets = TargetStore.from_dataset(ImagePoseDataset(dataset_json_path=path), device=device)
        return targets.q, targets.t, [targets.target(i, 1)[3] for i in range(len(targets))]
    raise ValueError(f"Unrecognized poses file format: {path}, Must be .pt or .json file")


def psnr_per_view(scene, decoded, q, t, infos, config):
    """the float PSNR of the decoded scene's picture against the original's, both clamped to [0, 1], per pose; read once"""
    module = Rast(config)
    out = torch.zeros(q.shape[0], dtype=torch.float32, device=q.device)

    def picture(s, i):
        return torch.clamp(module(Rast.GaussianPointCloudRasterisationInput(
            point_cloud=s.point_cloud, point_cloud_features=s.point_cloud_features, point_object_id=s.point_object_id,
            point_invalid_mask=s.point_invalid_mask, camera_info=infos[i], q_pointcloud_camera=q[i:i + 1].contiguous(),
            t_pointcloud_camera=t[i:i + 1].contiguous(), color_max_sh_band=3))[0], 0, 1)
    with torch.no_grad():
        for i in range(q.shape[0]):
            out[i] = 10 * torch.log10(1.0 / torch.mean((picture(decoded, i) - picture(scene, i)) ** 2))
    return [float(v) for v in out.cpu()]


if __name__ == "__main__":
    parser = argparse.ArgumentParser("Compress a Gaussian Point Cloud Scene")
    parser.add_argument("input", type=str, help="a parquet file with trained features")
    parser.add_argument("output", type=str, help="the compressed scene, .npz")
    parser.add_argument("--codes", type=int, default=4096)
    parser.add_argument("--iters", type=int, default=10)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--poses", type=str, default="")
    parser.add_argument("--image_height", type=int, default=544)
    parser.add_argument("--image_width", type=int, default=976)
    parser.add_argument("--camera_intrinsics", type=float, nargs=4, metavar=("FX", "FY", "CX", "CY"), default=(581.743, 581.743, 488.0, 272.0))
    parser.add_argument("--device", type=str, default="cuda")
    args = parser.parse_args()
    if not args.output.endswith(".npz"):
        parser.error("the output is a .npz file")

    scene = GaussianPointCloudScene.from_parquet(args.input, device=args.device)
    # the renderer's planes and sort key scale (GaussianPointRenderer)
    config = Rast.GaussianPointCloudRasterisationConfig(near_plane=0.8, far_plane=1000., depth_to_sort_key_scale=100.)
    kw = {}
    if args.poses:
        fx, fy, cx, cy = args.camera_intrinsics
        q, t, infos = load_poses(args.poses, scene.point_cloud.device, args.image_height, args.image_width,
                                 torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]]))
        kw = dict(weights="visibility", poses=(q, t, infos), rasterisation_config=config)
    compressed = scene.to_compressed(args.output, codes=args.codes, iters=args.iters, seed=args.seed, **kw)
    result = {"output": args.output, "rows": len(compressed), "codes": int(compressed.codebook.shape[0]),
              "bytes": os.path.getsize(args.output), "input_bytes": os.path.getsize(args.input),
              "distortion": [compressed.history[0], compressed.history[-1]]}
    if args.poses:
        decoded = GaussianPointCloudScene.from_compressed(args.output, device=args.device)
        config.rgb_only = True
        result["psnr"] = psnr_per_view(scene, decoded, q, t, infos, config)
    print(json.dumps(result))
