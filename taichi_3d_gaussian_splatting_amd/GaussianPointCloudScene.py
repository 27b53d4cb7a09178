"""The scene of the reference's training path (GaussianPointCloudScene.py): the point cloud and its 56 features as
parameters, the invalid mask and the object ids as buffers, rows preallocated for densification -- and initialize(), which
gives a bare x,y,z[,r,g,b] cloud its first features.  The one step of initialize() that the reference takes on the host
(scipy's cKDTree over a float64 copy, GaussianPointCloudScene.py:80-92) is knn.mean_neighbour_distance here: exact nearest
neighbours in HIP, on the tensors where they are.  Files go through scene_io.
"""
from dataclasses import dataclass
from typing import Optional, Union

import numpy as np
import torch
import torch.nn as nn

from . import knn, scene_io
from ._host import _ConfigBase

SH_C0 = 0.28209479177387814


def _logit(x: torch.Tensor) -> torch.Tensor:
    return torch.log(x / (1.0 - x))


def initial_features(point_cloud_features: torch.Tensor, point_invalid_mask: torch.Tensor, mean_neighbour_distance: torch.Tensor,
                     config, point_cloud_rgb=None) -> None:
    """Everything of the reference's initialize() behind the neighbour search (GaussianPointCloudScene.py:85-127), in place on
    point_cloud_features (M,56), on whichever device the tensors live.  mean_neighbour_distance: one value per VALID row, in
    row order; point_cloud_rgb: 0..255 per valid row or None."""
    valid = point_invalid_mask == 0
    ft = point_cloud_features
    with torch.no_grad():
        mean = torch.as_tensor(mean_neighbour_distance, dtype=torch.float32, device=ft.device)
        initial_covariance = torch.clip(mean * config.initial_covariance_ratio, 1e-6, config.max_initial_covariance)
        # s is the log of the scale
        ft[valid, 4:7] = torch.log(initial_covariance).unsqueeze(1)
        # rotation quaternion (x,y,z,w): random, normalised
        q = torch.rand_like(ft[:, 0:4])
        ft[:, 0:4] = q / torch.norm(q, dim=1, keepdim=True)
        ft[:, 7] = config.initial_alpha
        ft[:, 8:56] = 0.0
        ft[:, 8] = 1.0
        ft[:, 24] = 1.0
        ft[:, 40] = 1.0
        if point_cloud_rgb is not None:
            rgb = torch.as_tensor(np.asarray(point_cloud_rgb) if not isinstance(point_cloud_rgb, torch.Tensor) else point_cloud_rgb)
            rgb = torch.clamp(rgb.to(device=ft.device, dtype=torch.float32) / 255.0, 0.0, 0.99)
            for channel, column in enumerate((8, 24, 40)):
                ft[valid, column] = _logit(rgb[:, channel]) / SH_C0


class GaussianPointCloudScene(torch.nn.Module):

    @dataclass
    class PointCloudSceneConfig(_ConfigBase):
        num_of_features: int = 56
        max_num_points_ratio: Optional[float] = None
        add_sphere: bool = False
        sphere_radius_factor: float = 4.0
        num_points_sphere: int = 10000
        max_initial_covariance: Optional[float] = None
        initial_alpha: float = -2.0
        initial_covariance_ratio: float = 1.0

    def __init__(
        self,
        point_cloud: Union[np.ndarray, torch.Tensor],
        config: PointCloudSceneConfig,
        point_cloud_features: Optional[torch.Tensor] = None,
        point_object_id: Optional[torch.Tensor] = None,
    ):
        super().__init__()
        assert len(point_cloud.shape) == 2, "point_cloud must be a 2D array"
        assert point_cloud.shape[1] == 3, "point_cloud must have 3 columns(x,y,z)"
        if isinstance(point_cloud, np.ndarray):
            point_cloud = torch.tensor(point_cloud, dtype=torch.float32)
        num_points = point_cloud.shape[0]
        if config.max_num_points_ratio is not None:
            max_num_points = int(num_points * config.max_num_points_ratio)
            assert max_num_points > num_points, "max_num_points_ratio should be greater than 1.0"
            extra = max_num_points - num_points
            point_cloud = torch.cat([point_cloud, torch.zeros((extra, 3), dtype=point_cloud.dtype, device=point_cloud.device)], dim=0)
            if point_cloud_features is not None:
                point_cloud_features = torch.cat([point_cloud_features, torch.zeros(
                    (extra, config.num_of_features), dtype=point_cloud_features.dtype, device=point_cloud_features.device)], dim=0)
        self.point_cloud = nn.Parameter(point_cloud)
        self.config = config
        if point_cloud_features is None:
            point_cloud_features = torch.zeros(self.point_cloud.shape[0], self.config.num_of_features, device=point_cloud.device)
        self.point_cloud_features = nn.Parameter(point_cloud_features)
        self.register_buffer("point_invalid_mask", torch.zeros(self.point_cloud.shape[0], dtype=torch.int8, device=point_cloud.device))
        if point_object_id is None:
            point_object_id = torch.zeros(self.point_cloud.shape[0], dtype=torch.int32, device=point_cloud.device)
        self.register_buffer("point_object_id", point_object_id)
        if config.max_num_points_ratio is not None:
            self.point_invalid_mask[num_points:] = 1

    def forward(self):
        return self.point_cloud, self.point_cloud_features

    def initialize(self, point_cloud_rgb=None):
        """First features of a bare cloud: an isotropic Gaussian per valid point whose scale is the mean distance to its three
        nearest valid neighbours.  The search runs on the GPU; a module on the CPU is refused."""
        if not self.point_cloud.is_cuda:
            raise RuntimeError("GaussianPointCloudScene.initialize() searches the nearest neighbours on the GPU and has no CPU "
                               f"path: the scene is on {self.point_cloud.device}, move the module first (scene.to('cuda'))")
        with torch.no_grad():
            valid = self.point_invalid_mask == 0
            mean = knn.mean_neighbour_distance(self.point_cloud, 3, self.point_invalid_mask)[valid]
            initial_features(self.point_cloud_features, self.point_invalid_mask, mean, self.config, point_cloud_rgb)

    def _host_arrays(self):
        return (self.point_cloud.detach().cpu().numpy(), self.point_cloud_features.detach().cpu().numpy(),
                self.point_invalid_mask.cpu().numpy())

    def to_parquet(self, path: str):
        scene_io.save_parquet(path, *self._host_arrays())

    def to_ply(self, path: str):
        scene_io.save_inria_ply(path, *self._host_arrays())

    def to_compressed(self, path: str, **kw):
        """The valid rows behind an SH codebook, as one .npz (compression.compress(self, **kw).save(path)): about a seventh of
        the parquet.  The k-means runs on the GPU; a module on the CPU is refused.  -> the compression.CompressedScene written"""
        from . import compression
        compressed = compression.compress(self, **kw)
        compressed.save(path)
        return compressed

    @staticmethod
    def from_compressed(path: str, config=None, device="cuda"):
        """The scene a compressed file decodes to (compression.load(path).decode()), on `device`"""
        from . import compression
        config = config if config is not None else GaussianPointCloudScene.PointCloudSceneConfig()
        point_cloud, features = compression.load(path).decode()
        return GaussianPointCloudScene(point_cloud, config, point_cloud_features=features).to(device)

    @staticmethod
    def from_parquet(path: str, config=None, device="cuda"):
        """A file with feature columns loads as it is; a bare x,y,z[,r,g,b] cloud (with the sphere of config.add_sphere around
        it) is moved to `device` and initialised there, which needs a GPU."""
        config = config if config is not None else GaussianPointCloudScene.PointCloudSceneConfig()
        point_cloud, features, rgb = scene_io.load_parquet_columns(path)
        if features is not None:
            return GaussianPointCloudScene(point_cloud, config, point_cloud_features=torch.from_numpy(features)).to(device)
        if config.add_sphere:
            point_cloud, rgb = _add_sphere(point_cloud, rgb, config.sphere_radius_factor, config.num_points_sphere)
        scene = GaussianPointCloudScene(point_cloud, config).to(device)
        scene.initialize(point_cloud_rgb=rgb)
        return scene


def _add_sphere(point_cloud: np.ndarray, rgb: Optional[np.ndarray], radius_factor: float, num_points: int):
    """num_points random points on a sphere around the origin whose radius is half the largest extent of the cloud times
    radius_factor, mid-grey where the cloud has colours (GaussianPointCloudScene.py:212-239)"""
    far_distance = float((point_cloud.max(axis=0) - point_cloud.min(axis=0)).max()) / 2.0
    radius = far_distance * radius_factor
    phi = 2.0 * np.pi * np.random.rand(num_points)
    theta = np.arccos(2.0 * np.random.rand(num_points) - 1.0)
    points = np.stack([radius * np.sin(theta) * np.cos(phi), radius * np.sin(theta) * np.sin(phi), radius * np.cos(theta)], axis=1)
    point_cloud = np.concatenate([point_cloud, points.astype(np.float32)], axis=0)
    if rgb is not None:
        rgb = np.concatenate([rgb, np.full((num_points, 3), 255 // 2, dtype=rgb.dtype)], axis=0)
    return point_cloud, rgb
