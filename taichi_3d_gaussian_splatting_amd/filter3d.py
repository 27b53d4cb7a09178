"""The 3D smoothing filter of Mip-Splatting (include/gs_filter3d.h, csrc/k_filter3d.hip): every Gaussian gets an isotropic
low-pass whose width is the finest pixel footprint any training view had of it, so that a scene trained at one sampling rate
holds nothing a closer camera, a longer focal length or a higher resolution would show as needles and specks.

  views = view_table(train_dataset, device)                    # (V,16): R, t (camera from point cloud), fx, fy, cx, cy
  filt = Filter3D(Filter3DConfig(), scene, views)              # holds one rate per row of the scene; refresh() recomputes them
  features = filt.features(downsample_factor)                  # one autograd node over scene.point_cloud_features
  image, depth, count = rasterisation(input with point_cloud_features=features)
  loss.backward()                                              # the gradient reaches scene.point_cloud_features through the node
  filt.fuse_(scene)                                            # for export: the filter written into the scene, once

The rate of a row is the largest max(fx, fy) / depth over the views that see it (inside the frame grown by `margin` on every
side, beyond `near`); a valid row no view sees takes the smallest rate of any seen row, an invalid row +inf.  The filter's
standard deviation in the scene is k / rate, k = sqrt(variance) * factor with `factor` the downsample factor of the frame
being rendered.  A row is transformed as log-scales <- 0.5 log(exp(2 ls) + (k / rate)^2) and opacity <- opacity *
sqrt(det S^2 / det(S^2 + (k / rate)^2)); a rate of +inf leaves the row as it is.

apply() also normalises the quaternions of the rows it transforms IN `features` (the rasteriser's own in-place normalisation
would otherwise land on the copy, and the parameter's norm would drift under Adam).

There is no fallback path: every call goes through _native.call(), and a CPU tensor is refused.
"""
import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _native

VIEW_FLOATS = 16                                # GS_FILTER3D_VIEW_FLOATS
FEATURES = 56                                   # GS_FILTER3D_FEATURES
ROWS_PER_BLOCK = 256                            # GS_FILTER3D_ROWS_PER_BLOCK
MAX_POINTS = 2 ** 30                            # GS_FILTER3D_MAX_POINTS
MAX_VIEWS = 2 ** 20                             # GS_FILTER3D_MAX_VIEWS
DEFAULT_NEAR = 0.8                              # GaussianPointCloudRasterisationConfig.near_plane

_VP, _I32, _I64, _F32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
ARGTYPES = {
    # (ctx, point_cloud, point_invalid_mask, n_points, views, n_views, W, H, near, margin, rate_out, stream)
    "gs_filter3d_rate": [_VP, _VP, _VP, _I64, _VP, _I32, _I32, _I32, _F32, _F32, _VP, _VP],
    # (ctx, features, rate, n_points, k, features_out, stream)
    "gs_filter3d_apply": [_VP, _VP, _VP, _I64, _F32, _VP, _VP],
    # (ctx, grad_out, features, rate, n_points, k, grad_in, stream)
    "gs_filter3d_apply_backward": [_VP, _VP, _VP, _VP, _I64, _F32, _VP, _VP],
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


# ---- validation: reads no data, launches nothing ----------------------------------------------------------------------------
def _check(t, what, shape_tail, dtype, device=None, rows=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what} must be a tensor")
    if t.dim() != 1 + len(shape_tail) or tuple(t.shape[1:]) != tuple(shape_tail):
        raise ValueError(f"{what} must be (N,{','.join(str(s) for s in shape_tail)}), got {tuple(t.shape)}")
    if rows is not None and t.shape[0] != rows:
        raise ValueError(f"{what} has {t.shape[0]} rows, expected {rows}")
    if t.dtype != dtype:
        raise TypeError(f"{what} must be {str(dtype).replace('torch.', '')}, got {t.dtype}")
    if device is None:
        if not t.is_cuda:
            raise ValueError(f"the 3D filter runs on the GPU: {what} must be on a cuda/hip device (there is no CPU path)")
    elif t.device != device:
        raise ValueError(f"{what} is on {t.device}, expected {device}")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")


def check_k(k) -> float:
    k = float(k)
    if not math.isfinite(k) or k < 0.0:
        raise ValueError(f"k must be finite and >= 0, got {k!r}")
    return k


def filter_k(variance: float, factor) -> float:
    """sqrtf(variance) * factor in float32: the k of apply() for a frame at downsample factor `factor`"""
    return float(np.sqrt(np.float32(variance)) * np.float32(factor))


# ---- views ---------------------------------------------------------------------------------------------------------------
def view_rows(T_pointcloud_camera, camera_intrinsics) -> np.ndarray:
    """(V,4,4) camera poses in the point-cloud frame and (V,3,3) or (3,3) intrinsics -> the (V,16) float32 view table: the
    inverse pose (R = R_pc^T, t = -R_pc^T t_pc) in float64, rounded once, then fx, fy, cx, cy"""
    T = np.asarray(T_pointcloud_camera, dtype=np.float64).reshape(-1, 4, 4)
    K = np.asarray(camera_intrinsics, dtype=np.float64)
    K = np.broadcast_to(K, (T.shape[0], 3, 3)) if K.ndim == 2 else K.reshape(-1, 3, 3)
    if K.shape[0] != T.shape[0]:
        raise ValueError(f"{T.shape[0]} poses but {K.shape[0]} intrinsics")
    R = np.transpose(T[:, :3, :3], (0, 2, 1))
    t = -np.einsum("vij,vj->vi", R, T[:, :3, 3])
    rows = np.concatenate([R.reshape(-1, 9), t, K[:, 0, 0:1], K[:, 1, 1:2], K[:, 0, 2:3], K[:, 1, 2:3]], axis=1)
    return np.ascontiguousarray(rows, dtype=np.float32)


def view_table(source, camera_intrinsics=None, device="cuda") -> torch.Tensor:
    """-> the (V,16) float32 view table on `device`.  source: an ImagePoseDataset (every record's T_pointcloud_camera and the
    intrinsics its pictures are trained with: those of the file's real size) or (V,4,4) poses with (V,3,3) or (3,3)
    camera_intrinsics.  From a dataset whose pictures share one size the tensor carries it as .width and .height (the size the
    trainer renders at factor 1: cropped to multiples of 16).  Pictures over the trainer's 1600 pixels are refused: their
    autoscaled cameras are not built."""
    width = height = None
    if hasattr(source, "df"):
        import PIL.Image
        from .targets import MAX_RESOLUTION_TRAIN
        poses, intrinsics, sizes = [], [], set()
        for _, row in source.df.iterrows():
            with PIL.Image.open(row["image_path"]) as pil:
                w, h = pil.size                                  # the header only: nothing is decoded
            if h > MAX_RESOLUTION_TRAIN or w > MAX_RESOLUTION_TRAIN:
                raise ValueError(f"{row['image_path']}: the 3D filter for a picture over {MAX_RESOLUTION_TRAIN} pixels ({w}x{h}) is not "
                                 "supported (autoscaled views are not built)")
            k = np.array(row["camera_intrinsics"], dtype=np.float32).reshape(3, 3)       # float32, as ImagePoseDataset.load_raw scales it
            k[0, :] = k[0, :] * np.float32(w) / np.float32(row["camera_width"])
            k[1, :] = k[1, :] * np.float32(h) / np.float32(row["camera_height"])
            poses.append(np.array(row["T_pointcloud_camera"], dtype=np.float64).reshape(4, 4))
            intrinsics.append(k)
            sizes.add((w - w % 16, h - h % 16))
        rows = view_rows(np.stack(poses), np.stack(intrinsics)) if poses else np.zeros((0, VIEW_FLOATS), dtype=np.float32)
        if len(sizes) == 1:
            width, height = next(iter(sizes))
    else:
        if camera_intrinsics is None:
            raise ValueError("view_table: poses need camera_intrinsics")
        as_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        rows = view_rows(as_np(source), as_np(camera_intrinsics))
    table = torch.from_numpy(rows).to(device)
    table.width, table.height = width, height
    return table


def _check_views(views, device):
    if not isinstance(views, torch.Tensor):
        raise TypeError("views must be a tensor")
    if views.dim() != 2 or views.shape[1] != VIEW_FLOATS or views.shape[0] > MAX_VIEWS:
        raise ValueError(f"views must be (V,{VIEW_FLOATS}) with V <= {MAX_VIEWS}, got {tuple(views.shape)}")
    if views.dtype != torch.float32:
        raise TypeError(f"views must be float32, got {views.dtype}")
    if views.device != device:
        raise ValueError(f"views is on {views.device}, expected {device}")
    if not views.is_contiguous():
        raise ValueError("views must be contiguous")


# ---- the calls ----------------------------------------------------------------------------------------------------------
def sampling_rate(point_cloud, point_invalid_mask, views, W, H, near=DEFAULT_NEAR, margin=0.15, out=None):
    """gs_filter3d_rate: -> (N,) float32, the largest sampling rate of every row over the (V,16) `views` of W x H pixels; +inf
    for an invalid row, the smallest seen rate for a valid row no view sees, all +inf when nothing is seen.  out: an (N,)
    float32 tensor to write into.  No gradient."""
    _check(point_cloud, "point_cloud", (3,), torch.float32)
    dev, n = point_cloud.device, int(point_cloud.shape[0])
    _check(point_invalid_mask, "point_invalid_mask", (), torch.int8, dev, n)
    _check_views(views, dev)
    W, H, near, margin = int(W), int(H), float(near), float(margin)
    if W < 1 or H < 1:
        raise ValueError("W and H must be >= 1")
    if not math.isfinite(near) or not near > 0.0:
        raise ValueError("near must be finite and > 0")
    if not math.isfinite(margin) or margin < 0.0:
        raise ValueError("margin must be finite and >= 0")
    if n > MAX_POINTS:
        raise ValueError(f"more than {MAX_POINTS} rows")
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=dev)
    else:
        _check(out, "out", (), torch.float32, dev, n)
    _bind()
    _native.call("gs_filter3d_rate", dev, _native.shared_ctx(dev), _native.ptr(point_cloud.detach()), _native.ptr(point_invalid_mask), n,
                 _native.ptr(views), int(views.shape[0]), W, H, near, margin, _native.ptr(out))
    return out


def apply_forward(features, rate, k, out=None):
    """gs_filter3d_apply, no autograd: -> the (N,56) filtered rows in a buffer of their own.  The quaternions of the rows
    with k / rate > 0 are normalised in `features` itself."""
    _check(features, "features", (FEATURES,), torch.float32)
    dev, n = features.device, int(features.shape[0])
    _check(rate, "rate", (), torch.float32, dev, n)
    k = check_k(k)
    if out is None:
        out = torch.empty_like(features)
    else:
        _check(out, "out", (FEATURES,), torch.float32, dev, n)
    _bind()
    _native.call("gs_filter3d_apply", dev, _native.shared_ctx(dev), _native.ptr(features), _native.ptr(rate), n, k, _native.ptr(out))
    return out


def apply_backward(grad_out, features, rate, k, out=None):
    """gs_filter3d_apply_backward, no autograd: -> grad_in (N,56).  out: where to write; grad_out itself for in place."""
    _check(grad_out, "grad_out", (FEATURES,), torch.float32)
    dev, n = grad_out.device, int(grad_out.shape[0])
    _check(features, "features", (FEATURES,), torch.float32, dev, n)
    _check(rate, "rate", (), torch.float32, dev, n)
    k = check_k(k)
    if out is None:
        out = torch.empty_like(grad_out)
    else:
        _check(out, "out", (FEATURES,), torch.float32, dev, n)
    _bind()
    _native.call("gs_filter3d_apply_backward", dev, _native.shared_ctx(dev), _native.ptr(grad_out), _native.ptr(features), _native.ptr(rate), n, k,
                 _native.ptr(out))
    return out


class _Apply(torch.autograd.Function):
    """apply() as one autograd node.  The incoming gradient is left as it is (autograd may have handed it to others): the
    backward writes a buffer of its own."""

    @staticmethod
    def forward(ctx, features, rate, k):
        out = apply_forward(features.detach(), rate, k)
        ctx.save_for_backward(features, rate)
        ctx.k = k
        return out

    @staticmethod
    def backward(ctx, grad):
        features, rate = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        if grad.dtype != torch.float32:
            grad = grad.to(torch.float32)
        return apply_backward(grad.contiguous(), features.detach(), rate, ctx.k), None, None


def apply(features, rate, k):
    """-> the (N,56) rows of `features` under the filter k / rate, differentiable in features.  features: float32, contiguous,
    on a GPU (the scene's parameter: its quaternions are normalised in place, outside autograd); rate: (N,) float32 from
    sampling_rate(); k: filter_k(variance, factor).  The backward reads `features` again: step the optimiser after it."""
    _check(features, "features", (FEATURES,), torch.float32)
    _check(rate, "rate", (), torch.float32, features.device, int(features.shape[0]))
    return _Apply.apply(features, rate.detach(), check_k(k))


# ---- the filter of a scene ------------------------------------------------------------------------------------------------
@dataclass
class Filter3DConfig:
    """variance: of the filter, in square pixels of the frame being rendered (Mip-Splatting: 0.2).  interval: iterations
    between two refreshes of the rates in the trainer.  margin: by how much of its width and height a frame is grown on every
    side when a view is asked whether it sees a row.  near: the depth a row must exceed (None: the rasteriser's near plane)."""
    variance: float = 0.2
    interval: int = 100
    margin: float = 0.15
    near: Optional[float] = None

    def check(self):
        if not (math.isfinite(self.variance) and self.variance >= 0.0):
            raise ValueError("variance must be finite and >= 0")
        if isinstance(self.interval, bool) or not isinstance(self.interval, int) or self.interval < 1:
            raise ValueError("interval must be an integer >= 1")
        if not (math.isfinite(self.margin) and self.margin >= 0.0):
            raise ValueError("margin must be finite and >= 0")
        if self.near is not None and not (math.isfinite(self.near) and self.near > 0.0):
            raise ValueError("near must be finite and > 0")


class Filter3D:
    """The filter of a scene: `rate`, one float per row of the scene's full capacity (+inf until the first refresh()).
    scene: anything with point_cloud, point_cloud_features and point_invalid_mask on a GPU.  views: a (V,16) view table, or
    None for a filter that was loaded to be applied.  width, height: the pixels of the views at factor 1 (default: what
    view_table() found in its dataset)."""

    def __init__(self, config: Optional[Filter3DConfig], scene, views=None, width: Optional[int] = None, height: Optional[int] = None,
                 refresh: bool = True):
        self.config = Filter3DConfig() if config is None else config
        self.config.check()
        self.scene = scene
        device = scene.point_cloud.device
        if device.type != "cuda":
            raise ValueError("the 3D filter runs on the GPU: the scene must be on a cuda/hip device (there is no CPU path)")
        self.views = views
        self.width = width if width is not None else getattr(views, "width", None)
        self.height = height if height is not None else getattr(views, "height", None)
        if views is not None:
            _check_views(views, device)
            if self.width is None or self.height is None:
                raise ValueError("Filter3D needs the width and height of its views (the views of the table do not share one size)")
        self.near = DEFAULT_NEAR if self.config.near is None else float(self.config.near)
        self.rate = torch.full((scene.point_cloud.shape[0],), float("inf"), dtype=torch.float32, device=device)
        self.refreshes = 0
        if views is not None and refresh:
            self.refresh()

    def k(self, factor=1) -> float:
        return filter_k(self.config.variance, factor)

    def refresh(self):
        """the rates of every row of the scene as it is now, over the filter's views; no host read"""
        if self.views is None:
            raise ValueError("this filter has no views: it was loaded to be applied")
        with torch.no_grad():
            sampling_rate(self.scene.point_cloud, self.scene.point_invalid_mask, self.views, self.width, self.height, self.near,
                          self.config.margin, out=self.rate)
        self.refreshes += 1
        return self.rate

    def features(self, factor=1) -> torch.Tensor:
        """-> the scene's features under the filter for a frame at downsample factor `factor`: what the rasteriser is given in
        place of scene.point_cloud_features"""
        return apply(self.scene.point_cloud_features, self.rate, self.k(factor))

    def fuse_(self, scene=None, factor=1):
        """Writes the filtered log-scales and opacity logits into the scene's features in place (and normalises the quaternions
        of those rows): the scene any viewer renders as this package renders scene + filter at `factor`, Mip-Splatting's fused
        ply.  Once: a fused scene must not be filtered again."""
        scene = self.scene if scene is None else scene
        with torch.no_grad():
            features = scene.point_cloud_features.detach()
            fused = apply_forward(features, self.rate, self.k(factor))
            features[:, 4:8] = fused[:, 4:8]
        return scene

    def save(self, path: str):
        """A .pt of the rates of the scene's VALID rows, in row order -- the rows of the scene file written beside it -- with the
        filter's settings"""
        valid = self.scene.point_invalid_mask == 0
        torch.save(dict(rate=self.rate[valid].cpu(), variance=float(self.config.variance), interval=int(self.config.interval),
                        margin=float(self.config.margin), near=float(self.near), width=self.width, height=self.height,
                        views=None if self.views is None else self.views.cpu()), path)

    @classmethod
    def load(cls, path: str, scene, with_views: bool = False):
        """-> the filter of a file save() wrote, on `scene`: the stored rates go to the scene's valid rows (or to all rows, when
        there are as many).  with_views: keep the stored view table, so that refresh() works."""
        data = torch.load(path, map_location="cpu")
        rate = data["rate"]
        if rate.dim() != 1 or rate.dtype != torch.float32:
            raise ValueError(f"{path}: rate must be (N,) float32")
        config = Filter3DConfig(variance=float(data["variance"]), interval=int(data["interval"]), margin=float(data["margin"]),
                                near=float(data["near"]))
        device = scene.point_cloud.device
        views = data["views"].to(device) if with_views and data.get("views") is not None else None
        filt = cls(config, scene, views, width=data.get("width"), height=data.get("height"), refresh=False)
        n = int(scene.point_cloud.shape[0])
        if rate.shape[0] == n:
            filt.rate.copy_(rate)
        else:
            valid = scene.point_invalid_mask == 0
            if int(valid.sum().item()) != rate.shape[0]:
                raise ValueError(f"{path}: {rate.shape[0]} rates for a scene of {n} rows ({int(valid.sum().item())} valid)")
            filt.rate[valid] = rate.to(device)
        return filt
