"""Compressed scene files: the 45 higher-band SH coefficients of every Gaussian behind a codebook, the rest in half precision
(after Niedermayr et al., "Compressed 3D Gaussian Splatting for Accelerated Novel View Synthesis", CVPR 2024; Lee et al.,
"Compact 3D Gaussian Representation for Radiance Field"; LightGaussian).

  compressed = compress(scene, codes=4096, iters=10)         # k-means on the GPU (vq.py); weights="visibility" with poses=
  compressed.save("scene.npz");  load("scene.npz").decode()  # -> (point_cloud (N,3), point_cloud_features (N,56)) float32

Only valid rows are kept, in row order.  The container is numpy.savez_compressed with the keys

  format         str           "gsvq1"
  xyz            f32 (N,3)     unchanged
  q              f16 (N,4)     the quaternion AS STORED: the rasteriser does not normalise it, so neither does the codec
  log_scale      f16 (N,3)
  opacity_logit  f16 (N)
  sh_dc          f16 (N,3)     feature columns 8, 24, 40
  sh_index       u16 (N)       u8 when K <= 256
  codebook       f16 (K,45)    channel-major [R1..R15, G1..G15, B1..B15] = feature columns 9..23, 25..39, 41..55

36 bytes per Gaussian against 236, before deflate.  f16 is clamp(+-65504), then torch's round-to-nearest-even cast (a NaN
stays); decode is .float() and codebook.float()[sh_index].  The codec (encode, decode, save, load) runs on host arrays; the
clustering has no CPU path.  Not built: entropy coding, quantised positions, fine-tuning after quantisation, a trainer hook.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

FORMAT = "gsvq1"
F16_MAX = 65504.0
DC_COLUMNS = (8, 24, 40)
REST_COLUMNS = tuple(range(9, 24)) + tuple(range(25, 40)) + tuple(range(41, 56))
KEYS = ("format", "xyz", "q", "log_scale", "opacity_logit", "sh_dc", "sh_index", "codebook")
BYTES_PER_GAUSSIAN = 12 + 2 * (4 + 3 + 1 + 3) + 2


def to_f16(a) -> np.ndarray:
    """clamp(+-65504), then torch's round-to-nearest-even cast; a NaN stays a NaN"""
    t = torch.as_tensor(np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a), dtype=torch.float32)
    return torch.clamp(t, -F16_MAX, F16_MAX).to(torch.float16).numpy()


@dataclass
class CompressedScene:
    xyz: np.ndarray
    q: np.ndarray
    log_scale: np.ndarray
    opacity_logit: np.ndarray
    sh_dc: np.ndarray
    sh_index: np.ndarray
    codebook: np.ndarray
    history: Optional[list] = None          # the k-means distortion per iteration (compress() only; not stored)

    def __len__(self):
        return self.xyz.shape[0]

    def check(self):
        n, k = self.xyz.shape[0], self.codebook.shape[0]
        want = dict(xyz=(np.float32, (n, 3)), q=(np.float16, (n, 4)), log_scale=(np.float16, (n, 3)), opacity_logit=(np.float16, (n,)),
                    sh_dc=(np.float16, (n, 3)), sh_index=(np.uint8 if k <= 256 else np.uint16, (n,)), codebook=(np.float16, (k, 45)))
        for name, (dtype, shape) in want.items():
            a = getattr(self, name)
            if a.dtype != dtype or tuple(a.shape) != shape:
                raise ValueError(f"{name} must be {np.dtype(dtype).name} {shape}, got {a.dtype} {tuple(a.shape)}")
        if not 1 <= k <= 65536:
            raise ValueError(f"a codebook has 1..65536 rows, got {k}")
        if n and int(self.sh_index.max()) >= k:
            raise ValueError("sh_index points past the codebook")
        return self

    def decode(self, device=None):
        """-> (point_cloud (N,3), point_cloud_features (N,56)) float32 tensors (on `device`; the host by default)"""
        n = len(self)
        ft = torch.empty(n, 56, dtype=torch.float32)
        ft[:, 0:4] = torch.from_numpy(self.q).float()
        ft[:, 4:7] = torch.from_numpy(self.log_scale).float()
        ft[:, 7] = torch.from_numpy(self.opacity_logit).float()
        ft[:, list(DC_COLUMNS)] = torch.from_numpy(self.sh_dc).float()
        ft[:, list(REST_COLUMNS)] = torch.from_numpy(self.codebook).float()[torch.from_numpy(self.sh_index.astype(np.int64))]
        pc = torch.from_numpy(self.xyz).clone()
        return (pc, ft) if device is None else (pc.to(device), ft.to(device))

    def save(self, path):
        self.check()
        np.savez_compressed(path, format=np.array(FORMAT), **{k: getattr(self, k) for k in KEYS[1:]})

    def nbytes(self) -> int:
        """bytes of the arrays before deflate"""
        return int(sum(getattr(self, k).nbytes for k in KEYS[1:]))


def encode(point_cloud, point_cloud_features, sh_index, codebook) -> CompressedScene:
    """The codec alone, on host arrays or tensors: rows (N,3) and (N,56), one codebook row per Gaussian in sh_index (N), codebook
    (K,45) in the order of REST_COLUMNS.  A negative index is refused."""
    host = lambda a: np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a)
    pc, ft, idx, cb = host(point_cloud), host(point_cloud_features), host(sh_index), host(codebook)
    n, k = pc.shape[0], cb.shape[0]
    if pc.ndim != 2 or pc.shape[1] != 3 or tuple(ft.shape) != (n, 56) or tuple(idx.shape) != (n,) or cb.ndim != 2 or cb.shape[1] != 45:
        raise ValueError("need point_cloud (N,3), features (N,56), sh_index (N) and a codebook (K,45)")
    if not 1 <= k <= 65536:
        raise ValueError(f"a codebook has 1..65536 rows, got {k}")
    if n and (int(idx.min()) < 0 or int(idx.max()) >= k):
        raise ValueError("a row has no codebook entry (label -1: its SH coefficients are not finite) or one past the codebook")
    return CompressedScene(xyz=np.ascontiguousarray(pc, dtype=np.float32), q=to_f16(ft[:, 0:4]), log_scale=to_f16(ft[:, 4:7]),
                           opacity_logit=to_f16(ft[:, 7]), sh_dc=to_f16(ft[:, list(DC_COLUMNS)]),
                           sh_index=idx.astype(np.uint8 if k <= 256 else np.uint16), codebook=to_f16(cb)).check()


def load(path) -> CompressedScene:
    with np.load(path, allow_pickle=False) as z:
        if "format" not in z.files or str(z["format"]) != FORMAT:
            raise ValueError(f"{path} is not a {FORMAT} compressed scene (format: {str(z['format']) if 'format' in z.files else 'none'})")
        missing = [k for k in KEYS if k not in z.files]
        if missing:
            raise ValueError(f"{path} lacks {missing}")
        return CompressedScene(**{k: np.ascontiguousarray(z[k]) for k in KEYS[1:]}).check()


def _scene_tensors(scene):
    pc, ft = scene.point_cloud, scene.point_cloud_features
    for t, what in ((pc, "point_cloud"), (ft, "point_cloud_features")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"a scene is compressed on the GPU: {what} must be a tensor on a cuda/hip device (there is no CPU path)")
    pc, ft = pc.detach(), ft.detach()
    n = pc.shape[0]
    if pc.dtype != torch.float32 or ft.dtype != torch.float32 or tuple(pc.shape) != (n, 3) or tuple(ft.shape) != (n, 56):
        raise ValueError("a scene is point_cloud (N,3) and point_cloud_features (N,56), float32")
    mask = getattr(scene, "point_invalid_mask", None)
    mask = torch.zeros(n, dtype=torch.int8, device=pc.device) if mask is None else mask.to(device=pc.device, dtype=torch.int8)
    obj = getattr(scene, "point_object_id", None)
    obj = torch.zeros(n, dtype=torch.int32, device=pc.device) if obj is None else obj.to(device=pc.device, dtype=torch.int32)
    return pc.contiguous(), ft.contiguous(), mask.contiguous(), obj.contiguous()


def visibility_weights(scene, poses, rasterisation_config=None) -> torch.Tensor:
    """(N) float32: the blend weight alpha_i T_i of every Gaussian summed over the pixels of every pose -- how much of the
    pictures it is.  poses = (q_rows (F,K,4) or (F,4), t_rows (F,K,3) or (F,3), camera_info or one per pose).  Made with what
    exists: a frame kept by the rasteriser, one channel of ones rendered over it, and the gradient of that picture's sum."""
    from . import channels
    from .GaussianPointCloudRasterisation import GaussianPointCloudRasterisation as Rast
    pc, ft, mask, obj = _scene_tensors(scene)
    q_rows, t_rows, camera_info = poses
    q_rows = torch.as_tensor(q_rows, dtype=torch.float32).to(pc.device)
    t_rows = torch.as_tensor(t_rows, dtype=torch.float32).to(pc.device)
    if q_rows.dim() == 2:
        q_rows, t_rows = q_rows[:, None, :], t_rows[:, None, :]
    module = Rast(rasterisation_config if rasterisation_config is not None else Rast.GaussianPointCloudRasterisationConfig())
    total = torch.zeros(pc.shape[0], dtype=torch.float32, device=pc.device)
    infos = list(camera_info) if isinstance(camera_info, (list, tuple)) else [camera_info] * q_rows.shape[0]
    for i in range(q_rows.shape[0]):
        with torch.no_grad():
            module(Rast.GaussianPointCloudRasterisationInput(
                point_cloud=pc, point_cloud_features=ft, point_object_id=obj, point_invalid_mask=mask, camera_info=infos[i],
                q_pointcloud_camera=q_rows[i].contiguous(), t_pointcloud_camera=t_rows[i].contiguous(), color_max_sh_band=3), keep_frame=True)
        ones = torch.ones(pc.shape[0], 1, dtype=torch.float32, device=pc.device, requires_grad=True)
        channels.render_channels(ones, module.last_frame).sum().backward()
        total += ones.grad[:, 0]
    return total


def compress(scene, codes: int = 4096, iters: int = 10, weights=None, seed: int = 0, poses=None, rasterisation_config=None) -> CompressedScene:
    """scene: anything with point_cloud (N,3), point_cloud_features (N,56) and (optionally) point_invalid_mask on a GPU.
    weights: None (uniform), "visibility" (visibility_weights over poses=(q_rows, t_rows, camera_info)) or a tensor of one
    weight per row of the scene.  A scene with a non-finite SH coefficient raises ValueError."""
    from . import vq
    pc, ft, mask, _ = _scene_tensors(scene)
    if isinstance(weights, str):
        if weights != "visibility":
            raise ValueError(f"weights must be None, 'visibility' or a tensor, got {weights!r}")
        if poses is None:
            raise ValueError("weights='visibility' needs poses=(q_rows, t_rows, camera_info)")
        weights = visibility_weights(scene, poses, rasterisation_config)
    valid = mask == 0
    pc, ft = pc[valid], ft[valid]
    if weights is not None:
        weights = torch.as_tensor(weights, dtype=torch.float32).to(pc.device)
        if tuple(weights.shape) != tuple(valid.shape):
            raise ValueError(f"weights must have one entry per row of the scene ({valid.shape[0]}), got {tuple(weights.shape)}")
        weights = weights[valid].contiguous()
    if pc.shape[0] == 0:
        raise ValueError("the scene has no valid row")
    rest = ft[:, list(REST_COLUMNS)].contiguous()
    codebook, labels, history = vq.kmeans(rest, codes, iters=iters, weights=weights, seed=seed)
    if bool((labels < 0).any()):
        raise ValueError("a valid row has a non-finite SH coefficient: it has no nearest centroid")
    out = encode(pc, ft, labels, codebook)
    out.history = history
    return out
