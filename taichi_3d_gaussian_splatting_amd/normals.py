"""Rendered Gaussian normals and their consistency with the normal of the rendered depth (include/gs_normals.h,
csrc/k_normals.hip): the geometry term of 2DGS, GOF and PGSR, the one that needs no data -- no depth maps, no normal network.

  image, depth, _ = rast(input_data)                                                  # config.differentiable_depth = True
  R = rendered_normals(rast, scene, (q_pointcloud_camera, t_pointcloud_camera))       # (H,W,3), the blend of the Gaussians' normals
  c = normal_consistency(depth, R, camera_info.camera_intrinsics)                     # sum w (1 - n_depth . R / |R|) / sum w
  (loss + 0.05 * c).backward()
  c.terms                                                                             # {L, S_w, number selected, mean cos, 0, 0, 0, 0}

A Gaussian's normal is the shortest axis of its stored parametrisation (the column of R(q) of its smallest scale), in the camera
frame, turned to face the camera.  The consistency term reaches the rotations through the rendered normals (render_channels is
differentiable in its values) and positions, scales and opacities through the depth; the derivative of the rendered normal
through the blend weights is not taken.

There is no fallback path: every call goes through _native.call(), and a CPU tensor is refused.
"""
import ctypes as C
import math

import torch

from . import _native, _terms
from ._terms import check_plane
from .geometry import LOSS_TERMS, _GeometryTerm, _non_negative, _ptr, intrinsics_tuple

FEATURES = 56                                                       # GS_NORMALS_FEATURES
BLOCK = 256                                                         # GS_NORMALS_BLOCK
MAX_PIXELS = 715827200                                              # GS_NORMALS_MAX_PIXELS
FORWARD_LAUNCHES, BACKWARD_LAUNCHES = 2, 1                          # GS_NORMALS_*_LAUNCHES
MAX_ROWS = 2 ** 31 - 1 - BLOCK

_VP, _I32, _I64, _F32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
ARGTYPES = {
    # (ctx, point_cloud, features, point_object_id, q_pointcloud_camera, t_pointcloud_camera, N, K, normals, stream)
    "gs_gaussian_normals_forward": [_VP, _VP, _VP, _VP, _VP, _VP, _I64, _I32, _VP, _VP],
    # (ctx, point_cloud, features, point_object_id, q_pointcloud_camera, t_pointcloud_camera, N, K, grad_normals, grad_features, stream)
    "gs_gaussian_normals_backward": [_VP, _VP, _VP, _VP, _VP, _VP, _I64, _I32, _VP, _VP, _VP],
    # (ctx, D, R, w_p, H, W, fx, fy, cx, cy, max_rel_jump, min_length, terms, stream)
    "gs_normal_consistency_forward": [_VP, _VP, _VP, _VP, _I32, _I32, _F32, _F32, _F32, _F32, _F32, _F32, _VP, _VP],
    # (ctx, D, R, w_p, H, W, fx, fy, cx, cy, max_rel_jump, min_length, terms, upstream, grad_D, grad_R, stream)
    "gs_normal_consistency_backward": [_VP, _VP, _VP, _VP, _I32, _I32, _F32, _F32, _F32, _F32, _F32, _F32, _VP, _VP, _VP, _VP, _VP],
}
_bound = False


def _bind():
    """argtypes of the entry points, set once on the loaded library (they are not part of _native.SYMBOLS)"""
    global _bound
    if not _bound:
        L = _native.lib()
        for name, argtypes in ARGTYPES.items():
            if not hasattr(L, name):
                raise _native.NativeLibraryError(f"{_native.LIB_PATH} does not export {name}")
            fn = getattr(L, name)
            fn.argtypes, fn.restype = argtypes, C.c_int
        _bound = True


# ---- validation: reads no device data, launches nothing ---------------------------------------------------------------------
def _positive(value, what):
    value = float(value)
    if not (math.isfinite(value) and value > 0.0):
        raise ValueError(f"{what} must be finite and > 0, got {value}")
    return value


def _check_rows(tensor, what, columns, dtype=torch.float32, rows=None, device=None):
    if not isinstance(tensor, torch.Tensor):
        raise TypeError(f"{what} must be a tensor")
    if tensor.dtype != dtype:
        raise TypeError(f"{what} must be {dtype}, got {tensor.dtype}")
    shape = (tensor.shape[0],) + ((columns,) if columns else ()) if tensor.dim() >= 1 else None
    if shape is None or tuple(tensor.shape) != shape or (rows is not None and tensor.shape[0] != rows):
        want = f"({'N' if rows is None else rows}{',' + str(columns) if columns else ''})"
        raise ValueError(f"{what} must have shape {want}, got {tuple(tensor.shape)}")
    if not tensor.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    if device is not None and tensor.device != device:
        raise ValueError(f"{what} is on {tensor.device}, the point cloud on {device}")


def _check_gaussians(point_cloud, features, q_pointcloud_camera, t_pointcloud_camera, point_object_id, grad_normals=None):
    """what is wrong with a tensor is found before any device is looked at"""
    _check_rows(point_cloud, "point_cloud", 3)
    N = int(point_cloud.shape[0])
    if N > MAX_ROWS:
        raise ValueError(f"point_cloud has more than {MAX_ROWS} rows")
    _check_rows(features, "features", FEATURES, rows=N)
    _check_rows(q_pointcloud_camera, "q_pointcloud_camera", 4)
    K = int(q_pointcloud_camera.shape[0])
    if K < 1:
        raise ValueError("q_pointcloud_camera must hold at least one pose")
    _check_rows(t_pointcloud_camera, "t_pointcloud_camera", 3, rows=K)
    if point_object_id is not None:
        _check_rows(point_object_id, "point_object_id", 0, dtype=torch.int32, rows=N)
    if grad_normals is not None:
        _check_rows(grad_normals, "grad_normals", 3, rows=N)
    if not point_cloud.is_cuda:
        raise ValueError("Gaussian normals run on the GPU: point_cloud must be on a cuda/hip device (there is no CPU path)")
    for tensor, what in ((features, "features"), (q_pointcloud_camera, "q_pointcloud_camera"), (t_pointcloud_camera, "t_pointcloud_camera"),
                         (point_object_id, "point_object_id"), (grad_normals, "grad_normals")):
        if tensor is not None and tensor.device != point_cloud.device:
            raise ValueError(f"{what} is on {tensor.device}, the point cloud on {point_cloud.device}")
    return N, K


def check_rendered(rendered, what, depth, device=True):
    """Raise unless `rendered` is a contiguous float32 (H,W,3) tensor of the depth's size (and, with device=True, on its device)"""
    if not isinstance(rendered, torch.Tensor):
        raise TypeError(f"{what} must be a tensor")
    if rendered.dtype != torch.float32:
        raise TypeError(f"{what} must be float32, got {rendered.dtype}")
    if rendered.dim() != 3 or tuple(rendered.shape) != tuple(depth.shape) + (3,):
        raise ValueError(f"{what} must be (H,W,3) of the depth's size {tuple(depth.shape)}, as render_channels writes it, got {tuple(rendered.shape)}")
    if not rendered.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    if device and rendered.device != depth.device:
        raise ValueError(f"{what} is on {rendered.device}, the depth on {depth.device}")


def _check_consistency_inputs(depth, rendered, pixel_weight):
    for device in (False, True):
        check_plane(depth, "depth", device=device)
        if not device and depth.shape[0] * depth.shape[1] > MAX_PIXELS:
            raise ValueError(f"depth has more than {MAX_PIXELS} pixels")
        check_rendered(rendered, "rendered_normals", depth, device=device)
        if pixel_weight is not None:
            check_plane(pixel_weight, "pixel_weight", depth, device=device)


# ---- the calls --------------------------------------------------------------------------------------------------------------
def gaussian_normals_forward(point_cloud, features, q_pointcloud_camera, t_pointcloud_camera, point_object_id=None, out=None):
    """gs_gaussian_normals_forward, no autograd: -> (N,3) f32, every row written ((0,0,0) for a row that is not finite)"""
    N, K = _check_gaussians(point_cloud, features, q_pointcloud_camera, t_pointcloud_camera, point_object_id)
    if out is None:
        out = torch.empty((N, 3), dtype=torch.float32, device=point_cloud.device)
    else:
        _check_rows(out, "out", 3, rows=N, device=point_cloud.device)
    _bind()
    _native.call("gs_gaussian_normals_forward", point_cloud.device, _native.shared_ctx(point_cloud.device), _ptr(point_cloud), _ptr(features),
                 _ptr(point_object_id), _ptr(q_pointcloud_camera), _ptr(t_pointcloud_camera), N, K, _ptr(out))
    return out


def gaussian_normals_backward(point_cloud, features, q_pointcloud_camera, t_pointcloud_camera, point_object_id, grad_normals, out=None):
    """gs_gaussian_normals_backward, no autograd: -> grad_features (N,56), columns 0..3 the gradient to the quaternion, the rest 0"""
    N, K = _check_gaussians(point_cloud, features, q_pointcloud_camera, t_pointcloud_camera, point_object_id, grad_normals)
    if out is None:
        out = torch.empty((N, FEATURES), dtype=torch.float32, device=point_cloud.device)
    else:
        _check_rows(out, "out", FEATURES, rows=N, device=point_cloud.device)
    _bind()
    _native.call("gs_gaussian_normals_backward", point_cloud.device, _native.shared_ctx(point_cloud.device), _ptr(point_cloud), _ptr(features),
                 _ptr(point_object_id), _ptr(q_pointcloud_camera), _ptr(t_pointcloud_camera), N, K, _ptr(grad_normals), _ptr(out))
    return out


class _GaussianNormals(torch.autograd.Function):
    """differentiable in the features (their quaternion columns) only"""

    @staticmethod
    def forward(ctx, features, point_cloud, q_pointcloud_camera, t_pointcloud_camera, point_object_id):
        ctx.save_for_backward(features, point_cloud, q_pointcloud_camera, t_pointcloud_camera, point_object_id)
        return gaussian_normals_forward(point_cloud.detach(), features.detach(), q_pointcloud_camera.detach(), t_pointcloud_camera.detach(),
                                        point_object_id)

    @staticmethod
    def backward(ctx, grad_normals):
        features, point_cloud, q, t, point_object_id = ctx.saved_tensors
        if not ctx.needs_input_grad[0] or grad_normals is None:
            return None, None, None, None, None
        grad = gaussian_normals_backward(point_cloud.detach(), features.detach(), q.detach(), t.detach(), point_object_id,
                                         grad_normals.to(torch.float32).contiguous())
        return grad, None, None, None, None


def gaussian_normals(point_cloud, features, q_pointcloud_camera, t_pointcloud_camera, point_object_id=None) -> torch.Tensor:
    """-> (N,3) f32: the normal of every Gaussian in the camera frame of its object's pose (row point_object_id[i] of the (K,4)
    xyzw and (K,3) pose arrays; row 0 without ids): the column of R(q) of its smallest log-scale (features[:, 4:7]; ties to the
    smaller index), q = features[:, 0:4] as stored, normalised to unit length, rotated by the pose and turned so that it faces
    the camera.  (0,0,0) for a row that is not finite.  Differentiable in `features` (the quaternion columns: the axis choice and
    the sign are selections); no gradient goes to positions, scales or poses.  Contiguous float32 GPU tensors; queued on the
    current stream, no host synchronisation."""
    _check_gaussians(point_cloud, features, q_pointcloud_camera, t_pointcloud_camera, point_object_id)
    return _GaussianNormals.apply(features, point_cloud, q_pointcloud_camera, t_pointcloud_camera, point_object_id)


def normal_consistency_forward(depth, rendered, intrinsics, pixel_weight=None, max_rel_jump: float = 0.1, min_length: float = 0.5, terms=None):
    """gs_normal_consistency_forward, no autograd: -> the 8 terms {L, S_w, number selected, mean cos, 0, 0, 0, 0} on the device"""
    fx, fy, cx, cy = intrinsics_tuple(intrinsics)
    max_rel_jump, min_length = _non_negative(max_rel_jump, "max_rel_jump"), _positive(min_length, "min_length")
    _check_consistency_inputs(depth, rendered, pixel_weight)
    if terms is None:
        terms = torch.empty(LOSS_TERMS, dtype=torch.float32, device=depth.device)
    _bind()
    H, W = int(depth.shape[0]), int(depth.shape[1])
    _native.call("gs_normal_consistency_forward", depth.device, _native.shared_ctx(depth.device), depth.data_ptr(), rendered.data_ptr(),
                 _ptr(pixel_weight), H, W, fx, fy, cx, cy, max_rel_jump, min_length, terms.data_ptr())
    return terms


def normal_consistency_backward(depth, rendered, intrinsics, pixel_weight, max_rel_jump: float, min_length: float, terms, upstream=None,
                                out_depth=None, out_rendered=None):
    """gs_normal_consistency_backward, no autograd: -> (grad_depth (H,W), grad_rendered (H,W,3)), every element written by one
    launch.  upstream: one float32 on the device (None: 1)"""
    fx, fy, cx, cy = intrinsics_tuple(intrinsics)
    max_rel_jump, min_length = _non_negative(max_rel_jump, "max_rel_jump"), _positive(min_length, "min_length")
    _check_consistency_inputs(depth, rendered, pixel_weight)
    if out_depth is None:
        out_depth = torch.empty_like(depth)
    else:
        check_plane(out_depth, "out_depth", depth)
    if out_rendered is None:
        out_rendered = torch.empty_like(rendered)
    else:
        check_rendered(out_rendered, "out_rendered", depth)
    _terms.check_upstream(upstream, depth)
    _bind()
    H, W = int(depth.shape[0]), int(depth.shape[1])
    _native.call("gs_normal_consistency_backward", depth.device, _native.shared_ctx(depth.device), depth.data_ptr(), rendered.data_ptr(),
                 _ptr(pixel_weight), H, W, fx, fy, cx, cy, max_rel_jump, min_length, terms.data_ptr(), _ptr(upstream), out_depth.data_ptr(),
                 out_rendered.data_ptr())
    return out_depth, out_rendered


class _Consistency(torch.autograd.Function):
    """one node, differentiable in the depth and in the rendered normals (_terms._DepthTerm is depth-only)"""

    @staticmethod
    def forward(ctx, depth, rendered, pixel_weight, scalars):
        ctx.scalars = scalars
        terms = normal_consistency_forward(depth.detach(), rendered.detach(), pixel_weight=pixel_weight, **scalars)
        ctx.save_for_backward(depth, rendered, pixel_weight, terms)
        ctx.mark_non_differentiable(terms)
        return terms[0], terms

    @staticmethod
    def backward(ctx, grad_loss, _grad_terms):
        depth, rendered, pixel_weight, terms = ctx.saved_tensors
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]) or grad_loss is None:
            return None, None, None, None
        grad_depth, grad_rendered = normal_consistency_backward(depth.detach(), rendered.detach(), pixel_weight=pixel_weight, **ctx.scalars,
                                                                terms=terms, upstream=_terms.upstream_of(grad_loss))
        return (grad_depth if ctx.needs_input_grad[0] else None), (grad_rendered if ctx.needs_input_grad[1] else None), None, None


def normal_consistency_checked(depth, rendered, intrinsics, pixel_weight, max_rel_jump, min_length):
    """normal_consistency() of checked arguments and an (fx, fy, cx, cy) tuple: what a caller that fixed them once calls per step"""
    loss, terms = _Consistency.apply(depth, rendered, pixel_weight, dict(intrinsics=intrinsics, max_rel_jump=max_rel_jump, min_length=min_length))
    loss.terms = terms
    return loss


def normal_consistency(depth, rendered_normals, intrinsics, pixel_weight=None, max_rel_jump: float = 0.1, min_length: float = 0.5):
    """-> the scalar sum w (1 - n . h) / sum w over the selected pixels: n the depth-derived normal (geometry.depth_normals) of the
    contiguous float32 (H,W) GPU plane `depth`, h = R / |R| of the (H,W,3) `rendered_normals` (render_channels of
    gaussian_normals: the alpha-weighted blend, not normalised), w the pixel weight.  A pixel is selected iff its depth normal
    exists (not across a depth change of more than max_rel_jump times the depth; 0: no such test), |R| >= min_length (a thin
    blend, or one whose normals cancelled, is left out) and w > 0.  One autograd node, differentiable in `depth` and in
    `rendered_normals`.  The result's `.terms` is the (8,) tensor {L, S_w, number selected, mean n . h, 0, 0, 0, 0} on the device."""
    intrinsics = intrinsics_tuple(intrinsics)
    max_rel_jump, min_length = _non_negative(max_rel_jump, "max_rel_jump"), _positive(min_length, "min_length")
    _check_consistency_inputs(depth, rendered_normals, pixel_weight)
    return normal_consistency_checked(depth, rendered_normals, intrinsics, pixel_weight, max_rel_jump, min_length)


def unit_normals(rendered: torch.Tensor, min_length: float = 0.5) -> torch.Tensor:
    """(H,W,3) rendered normals -> (3,H,W): R / |R| where |R| >= min_length, (0,0,0) elsewhere -- what geometry.normals_to_uint8
    encodes.  Plain torch on whichever device the normals are."""
    length = rendered.norm(dim=2, keepdim=True)
    usable = length >= min_length
    return torch.where(usable, rendered / torch.where(usable, length, torch.ones_like(length)), torch.zeros_like(rendered)).permute(2, 0, 1).contiguous()


def _scene_tensors(scene_or_tensors):
    """(point_cloud, features, point_object_id or None) of a GaussianPointCloudScene or of a tuple of two or three tensors"""
    if isinstance(scene_or_tensors, (tuple, list)):
        if len(scene_or_tensors) not in (2, 3):
            raise ValueError("scene_or_tensors must be a scene or (point_cloud, features[, point_object_id])")
        return tuple(scene_or_tensors) + (None,) * (3 - len(scene_or_tensors))
    scene = scene_or_tensors
    if not hasattr(scene, "point_cloud") or not hasattr(scene, "point_cloud_features"):
        raise ValueError("scene_or_tensors must be a scene or (point_cloud, features[, point_object_id])")
    return scene.point_cloud, scene.point_cloud_features, getattr(scene, "point_object_id", None)


def rendered_normals(rast, scene_or_tensors, pose, frame=None) -> torch.Tensor:
    """-> (H,W,3): rast.render_channels(gaussian_normals(...), frame), the Gaussians' normals blended over the frame (default:
    the frame of rast's last forward) with the colour's own weights.  scene_or_tensors: a GaussianPointCloudScene or
    (point_cloud, features[, point_object_id]); pose: (q_pointcloud_camera (K,4), t_pointcloud_camera (K,3)), as the forward
    that made the frame was given.  Differentiable in the features' quaternion columns."""
    point_cloud, features, point_object_id = _scene_tensors(scene_or_tensors)
    if not isinstance(pose, (tuple, list)) or len(pose) != 2:
        raise ValueError("pose must be (q_pointcloud_camera, t_pointcloud_camera)")
    normals = gaussian_normals(point_cloud, features, pose[0], pose[1], point_object_id)
    return rast.render_channels(normals, frame)


# ---- the trainer's term -------------------------------------------------------------------------------------------------------
class ConsistencyTerm(_GeometryTerm):
    """normal_consistency of the rendered depth with the rendered Gaussian normals of the same frame.  Beyond what value() is
    given it needs the frame the rasteriser made in this step, the scene's tensors and the view's pose: it keeps the trainer
    (bind) and reads trainer.rasterisation.last_frame, trainer.scene and trainer.current_pose.  It needs no data."""
    name = "consistency"

    def __init__(self, config):
        super().__init__(config)
        self.trainer = None
        self._intrinsics = {}                       # (split, view, factor) -> (fx, fy, cx, cy), read by the host once

    def bind(self, trainer):
        self.trainer = trainer

    def value(self, split, view, downsample_factor, image_depth, image_gt, camera_info, pixel_weight):
        if self.trainer is None:
            raise RuntimeError("ConsistencyTerm.value() before bind(trainer)")
        key = (split, view, downsample_factor)
        intrinsics = self._intrinsics.get(key)
        if intrinsics is None:
            intrinsics = self._intrinsics[key] = intrinsics_tuple(camera_info.camera_intrinsics)
        trainer = self.trainer
        rendered = rendered_normals(trainer.rasterisation, trainer.scene, trainer.current_pose)
        _check_consistency_inputs(image_depth, rendered, pixel_weight)
        return normal_consistency_checked(image_depth, rendered, intrinsics, pixel_weight, float(self.config.consistency_max_rel_jump),
                                          float(self.config.consistency_min_length))
