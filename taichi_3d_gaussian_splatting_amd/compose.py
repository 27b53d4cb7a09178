"""Composing and baking scenes (include/gs_compose.h, csrc/k_compose.hip).

scene_bake() is the library call: one similarity transform (unit quaternion, translation, uniform scale) applied to the rows
of a scene -- positions, covariance quaternions, log-scales and the SH colour coefficients of bands 1..3 -- written into a row
range of the outputs.  SceneComposition holds several scenes as one point set with one pose row per object, the way the
reference's visualiser feeds the operator (visualizer.py:_merge_scenes), keeps a placement per object, hides and shows
objects, turns a camera pose into the K pose rows the rasteriser wants, and bakes the whole composition into one ordinary
scene in the world frame, which the visualiser cannot do.

The SH rotation matrices are made here, on the host, in float64 (sh_rotation_matrices) and rounded once; the kernel
evaluates no basis function.  There is no fallback path: every bake goes through _native.call(), and CPU tensors are refused.
"""
import ctypes as C
import functools
import os
from dataclasses import dataclass
from typing import Dict, Sequence, Tuple

import numpy as np
import torch

from . import _native
from .GaussianPointCloudScene import GaussianPointCloudScene
from .utils import quaternion_multiply_torch, quaternion_to_rotation_matrix_torch

FEATURES = 56           # GS_BAKE_FEATURES
SH_FLOATS = 84          # GS_BAKE_SH_FLOATS: M_0 (1x1), M_1 (3x3), M_2 (5x5), M_3 (7x7), row-major
ROWS_PER_BLOCK = 64     # GS_BAKE_ROWS_PER_BLOCK
BANDS = ((0, 1), (1, 4), (4, 9), (9, 16))      # the coefficients of band l

_VP, _I64, _F32 = C.c_void_p, C.c_int64, C.c_float
ARGTYPES = {
    # (ctx, xyz_in, features_in, n, q_A, t_A, scale, sh_matrices, xyz_out, features_out, row_offset, stream)
    "gs_scene_bake": [_VP, _VP, _VP, _I64, _VP, _VP, _F32, _VP, _VP, _VP, _I64, _VP],
}
_bound = False


def _bind():
    """argtypes of the entry point, set once on the loaded library (it is not part of _native.SYMBOLS)"""
    global _bound
    if not _bound:
        L = _native.lib()
        for name, argtypes in ARGTYPES.items():
            if not hasattr(L, name):
                raise _native.NativeLibraryError(f"{_native.LIB_PATH} does not export {name}")
            fn = getattr(L, name)
            fn.argtypes, fn.restype = argtypes, C.c_int
        _bound = True


# ---- the colour basis and its rotation (host, float64) -------------------------------------------------------------------
def sh_basis(d: np.ndarray) -> np.ndarray:
    """(n,3) unit directions -> (n,16) float64: the 16 functions the rasteriser shades with (gs_sh16 in csrc/gs_point_math.h),
    signs included: they are not the textbook ones"""
    d = np.asarray(d, np.float64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    return np.stack([
        np.full_like(x, 0.28209479177387814),
        -0.48860251190291987 * y, 0.48860251190291987 * z, -0.48860251190291987 * x,
        1.0925484305920792 * x * y, -1.0925484305920792 * y * z, 0.94617469575755997 * z * z - 0.31539156525251999,
        -1.0925484305920792 * x * z, 0.54627421529603959 * x * x - 0.54627421529603959 * y * y,
        0.59004358992664352 * y * (-3.0 * x * x + y * y), 2.8906114426405538 * x * y * z,
        0.45704579946446572 * y * (1.0 - 5.0 * z * z), 0.3731763325901154 * z * (5.0 * z * z - 3.0),
        0.45704579946446572 * x * (1.0 - 5.0 * z * z), 1.4453057213202769 * z * (x * x - y * y),
        0.59004358992664352 * x * (-x * x + 3.0 * y * y)], axis=1)


def _sample_directions(n: int = 96) -> np.ndarray:
    """n fixed, well spread unit directions (a Fibonacci spiral): the least-squares systems below are far over-determined"""
    i = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / n
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def quaternion_to_matrix(q) -> np.ndarray:
    """xyzw, normalised here -> (3,3) float64"""
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(np.asarray(q, np.float64))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def sh_rotation_matrices(R: np.ndarray) -> np.ndarray:
    """(3,3) rotation -> (84,) float64: M_0 | M_1 | M_2 | M_3 row-major, with Y_l(R d) = M_l Y_l(d) for sh_basis.  Each band is
    closed under rotation and M_l is orthogonal, so coefficients f' = M_l f reproduce the colour of f in the rotated frame:
    sum f'_k Y_k(R d) = sum f_k Y_k(d).  M_l^T = lstsq(Y_l(D), Y_l(D R^T)) over fixed sample directions D."""
    D = _sample_directions()
    Y, Yr = sh_basis(D), sh_basis(D @ np.asarray(R, np.float64).T)
    out = [np.ones(1)]                                  # band 0 is a constant
    for lo, hi in BANDS[1:]:
        Mt = np.linalg.lstsq(Y[:, lo:hi], Yr[:, lo:hi], rcond=None)[0]
        out.append(Mt.T.reshape(-1))
    return np.concatenate(out)


@functools.lru_cache(maxsize=64)
def _sh_arguments(q: tuple):
    """the f32 matrices of a (normalised) placement quaternion as the library takes them; a placement is baked many times"""
    return (C.c_float * SH_FLOATS)(*sh_rotation_matrices(quaternion_to_matrix(q)).astype(np.float32))


def _placement(q, t, scale) -> Tuple[np.ndarray, np.ndarray, float]:
    host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    q, t = np.asarray(host(q), np.float64).reshape(4), np.asarray(host(t), np.float64).reshape(3)
    norm = float(np.linalg.norm(q))
    if not np.isfinite(norm) or norm <= 0.0:
        raise ValueError("a placement quaternion must have a finite norm > 0")
    if not np.all(np.isfinite(t)):
        raise ValueError("a placement translation must be finite")
    scale = float(scale)
    if not np.isfinite(scale) or scale <= 0.0:
        raise ValueError(f"a placement scale must be finite and > 0, got {scale}")
    return q / norm, t, scale


def scene_bake(point_cloud: torch.Tensor, point_cloud_features: torch.Tensor, q, t, scale: float = 1.0, out_point_cloud=None,
               out_features=None, row_offset: int = 0):
    """-> (out_point_cloud, out_features): rows [row_offset, row_offset + n) of the outputs are the n input rows under the
    similarity p -> scale * R(q) p + t (q xyzw, normalised here).  The inputs are contiguous f32 (n,3) and (n,56) on a GPU; the
    outputs (new tensors of n rows by default) contiguous f32 of at least row_offset + n rows on the same device, and may not
    overlap the inputs.  Queued on the current stream; no host synchronisation."""
    _bind()
    q, t, scale = _placement(q, t, scale)
    pc, ft = point_cloud, point_cloud_features
    if not (isinstance(pc, torch.Tensor) and isinstance(ft, torch.Tensor)) or not pc.is_cuda or not ft.is_cuda:
        raise ValueError("scenes are baked on the GPU: move the tensors to a cuda/hip device first (there is no CPU path)")
    n = pc.shape[0]
    if pc.dtype != torch.float32 or ft.dtype != torch.float32 or pc.dim() != 2 or tuple(pc.shape) != (n, 3) or \
            tuple(ft.shape) != (n, FEATURES) or not pc.is_contiguous() or not ft.is_contiguous() or ft.device != pc.device:
        raise ValueError(f"need contiguous float32 point_cloud (n,3) and features (n,{FEATURES}) on one device")
    row_offset = int(row_offset)
    if out_point_cloud is None and out_features is None:
        if row_offset < 0:
            raise ValueError("row_offset must not be negative")
        out_point_cloud = torch.empty((row_offset + n, 3), dtype=torch.float32, device=pc.device)
        out_features = torch.empty((row_offset + n, FEATURES), dtype=torch.float32, device=pc.device)
    for o, width in ((out_point_cloud, 3), (out_features, FEATURES)):
        if not isinstance(o, torch.Tensor) or o.dtype != torch.float32 or o.device != pc.device or o.dim() != 2 or o.shape[1] != width \
                or not o.is_contiguous() or o.shape[0] < row_offset + n:
            raise ValueError(f"the outputs must be contiguous float32 (>= row_offset + n, {width}) tensors on {pc.device}")
    q32, t32 = (C.c_float * 4)(*q.astype(np.float32)), (C.c_float * 3)(*t.astype(np.float32))
    sh32 = _sh_arguments(tuple(float(v) for v in q))
    # data_ptr() and not _native.ptr(): an empty tensor must still reach the library's own checks as it is
    _native.call("gs_scene_bake", pc.device, _native.shared_ctx(pc.device), _native.ptr(pc), _native.ptr(ft), n, q32, t32,
                 float(np.float32(scale)), sh32, out_point_cloud.data_ptr() or None, out_features.data_ptr() or None, row_offset)
    return out_point_cloud, out_features


class SceneComposition:
    """Several scenes held as one: rows concatenated in order on the device, point_object_id = index of the source, one
    placement A_k = (q, t, scale) per object (object frame -> world frame; the identity at first) and one visibility flag.

    sources: GaussianPointCloudScene objects, (point_cloud, features[, point_invalid_mask]) tuples of arrays or tensors, or
    paths of parquet files with trained features or of compressed scenes (.npz, compression.py).

      scene                  the merged GaussianPointCloudScene (object frames, as loaded); its point_invalid_mask carries the
                             sources' masks and the hidden objects
      extra_scene_info_dict  the reference's ExtraSceneInfo per object: start_offset, end_offset, center, visible
      camera_rows(q, t)      the K pose rows q_pointcloud_camera / t_pointcloud_camera of the rasteriser for one camera pose
      bake()                 one ordinary scene in the world frame, point_object_id zero

    Rendering bake() under a pose T_cam shows what the composition shows under camera_rows(T_cam) -- for a UNIT pose
    quaternion.  Placement quaternions are normalised on entry; a camera quaternion is passed on as it is, and a non-unit one
    is not a rotation in the rasteriser's rotation_matrix_from_quaternion (it also scales), so the two pictures then differ:
    by up to 0.03 for the slightly non-unit pose the parity tests use on purpose."""

    @dataclass
    class ExtraSceneInfo:
        start_offset: int
        end_offset: int
        center: torch.Tensor
        visible: bool

    def __init__(self, sources: Sequence, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"a SceneComposition lives on a GPU, got {self.device} (there is no CPU path)")
        _bind()
        parts = [self._load(s) for s in sources]
        if not parts:
            raise ValueError("a SceneComposition needs at least one scene")
        sizes = [p[0].shape[0] for p in parts]
        ends = np.cumsum(sizes).tolist()
        starts = [0] + ends[:-1]
        point_cloud = torch.cat([p[0] for p in parts], dim=0)
        features = torch.cat([p[1] for p in parts], dim=0)
        self._source_mask = torch.cat([p[2] for p in parts], dim=0)
        object_id = torch.cat([torch.full((n,), k, dtype=torch.int32, device=self.device) for k, n in enumerate(sizes)], dim=0)
        self.scene = GaussianPointCloudScene(point_cloud, GaussianPointCloudScene.PointCloudSceneConfig(max_num_points_ratio=None),
                                             point_cloud_features=features, point_object_id=object_id)
        self.scene.point_invalid_mask.copy_(self._source_mask)
        self.extra_scene_info_dict: Dict[int, SceneComposition.ExtraSceneInfo] = {
            k: self.ExtraSceneInfo(start_offset=int(a), end_offset=int(b),
                                   center=parts[k][0].mean(dim=0) if b > a else torch.zeros(3, device=self.device), visible=True)
            for k, (a, b) in enumerate(zip(starts, ends))}
        self.placements = [(np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3), 1.0) for _ in parts]
        self._rows = None           # (conj(q_A) (K,4), t_A (K,3)) float64 on the device, made on demand

    def _load(self, source):
        if isinstance(source, (str, bytes)) or hasattr(source, "__fspath__"):
            from . import scene_io
            if os.fsdecode(source).endswith(".npz"):        # a compressed scene (compression.py)
                from . import compression
                source = compression.load(os.fsdecode(source)).decode()
            else:
                source = scene_io.load_parquet(str(source))
        if isinstance(source, GaussianPointCloudScene):
            source = (source.point_cloud.detach(), source.point_cloud_features.detach(), source.point_invalid_mask)
        as_f32 = lambda a: torch.as_tensor(a).detach().to(device=self.device, dtype=torch.float32).contiguous()
        pc, ft = as_f32(source[0]), as_f32(source[1])
        if pc.dim() != 2 or pc.shape[1] != 3 or tuple(ft.shape) != (pc.shape[0], FEATURES):
            raise ValueError(f"a scene is a (n,3) point cloud and its (n,{FEATURES}) features")
        if len(source) > 2 and source[2] is not None:
            mask = torch.as_tensor(source[2]).to(device=self.device, dtype=torch.int8)
        else:
            mask = torch.zeros(pc.shape[0], dtype=torch.int8, device=self.device)
        return pc, ft, mask

    def __len__(self):
        return len(self.placements)

    def place(self, k: int, q, t, scale: float = 1.0):
        """the placement of object k: p_world = scale * R(q) p_object + t; q xyzw, normalised here"""
        self.placements[k] = _placement(q, t, scale)
        self._rows = None

    def set_visible(self, k: int, visible: bool):
        """hide or show object k: writes its range of the merged scene's point_invalid_mask (the visualiser's h / p keys)"""
        info = self.extra_scene_info_dict[k]
        info.visible = bool(visible)
        a, b = info.start_offset, info.end_offset
        if visible:
            self.scene.point_invalid_mask[a:b] = self._source_mask[a:b]
        else:
            self.scene.point_invalid_mask[a:b] = 1

    def camera_rows(self, q_cam: torch.Tensor, t_cam: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """One camera pose T_cam = (q_cam (4) or (1,4), t_cam (3) or (1,3)), world <- camera -> (K,4), (K,3) f32 on the device:
        row k is A_k^-1 o T_cam, object k's frame <- camera, which is what the rasteriser takes as q_pointcloud_camera /
        t_pointcloud_camera.  F > 1 poses ((F,4), (F,3)) give (F,K,4), (F,K,3).  Computed in float64, rounded once; with the
        identity placement the row is the pose itself, bit for bit.  A scale other than 1 cannot be a pose row: bake() instead."""
        for k, (_, _, scale) in enumerate(self.placements):
            if scale != 1.0:
                raise ValueError(f"object {k} is placed with scale {scale}: a scale cannot be expressed as a pose row of the "
                                 "rasteriser; bake() the composition and render the baked scene instead")
        if self._rows is None:
            qa = torch.tensor(np.stack([p[0] * [-1.0, -1.0, -1.0, 1.0] for p in self.placements]), dtype=torch.float64, device=self.device)
            ta = torch.tensor(np.stack([p[1] for p in self.placements]), dtype=torch.float64, device=self.device)
            self._rows = (qa, quaternion_to_rotation_matrix_torch(qa), ta)
        qa, Ra, ta = self._rows                                            # conj(q_A) (K,4), R_A^T (K,3,3), t_A (K,3)
        q = q_cam.to(device=self.device, dtype=torch.float64).reshape(-1, 1, 4)
        t = t_cam.to(device=self.device, dtype=torch.float64).reshape(-1, 1, 3)
        q_rows = quaternion_multiply_torch(qa.unsqueeze(0).expand(q.shape[0], -1, -1), q.expand(-1, qa.shape[0], -1))
        t_rows = torch.einsum("kij,fkj->fki", Ra, t - ta.unsqueeze(0))
        q_rows, t_rows = q_rows.to(torch.float32), t_rows.to(torch.float32)
        if q.shape[0] == 1:
            return q_rows[0].contiguous(), t_rows[0].contiguous()
        return q_rows.contiguous(), t_rows.contiguous()

    def bake(self) -> GaussianPointCloudScene:
        """-> one GaussianPointCloudScene in the world frame: every object under its placement, rows in the merged order,
        point_object_id zero, the merged scene's point_invalid_mask (hidden objects stay hidden; to_parquet drops them).
        One launch per object into its row range; no concatenation pass."""
        pc, ft = self.scene.point_cloud.detach(), self.scene.point_cloud_features.detach()
        out_pc, out_ft = torch.empty_like(pc), torch.empty_like(ft)
        for k, (q, t, scale) in enumerate(self.placements):
            info = self.extra_scene_info_dict[k]
            a, b = info.start_offset, info.end_offset
            if b > a:
                scene_bake(pc[a:b], ft[a:b], q, t, scale, out_pc, out_ft, row_offset=a)
        baked = GaussianPointCloudScene(out_pc, GaussianPointCloudScene.PointCloudSceneConfig(max_num_points_ratio=None),
                                        point_cloud_features=out_ft)
        baked.point_invalid_mask.copy_(self.scene.point_invalid_mask)
        return baked
