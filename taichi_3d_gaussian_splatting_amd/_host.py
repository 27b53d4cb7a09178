"""What the operator, the staged path and the controller share above the binding: the config base class, the tensor checks,
the argument structs of a scene and a view, the contexts of one operator instance and the frame ticket.  The library
calls themselves go through _native.call()."""
import torch

from . import _native

try:  # the reference mixes in dataclass_wizard.YAMLWizard (RAST:777); optional here
    from dataclass_wizard import YAMLWizard as _ConfigBase
except Exception:  # pragma: no cover - not installed in the build image
    class _ConfigBase:
        pass

_TORCH_DTYPES = {"float32": torch.float32, "int32": torch.int32, "int64": torch.int64, "int8": torch.int8}


def _require(t: torch.Tensor, name: str, dtype, shape_tail, device=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_cuda:
        raise ValueError(f"{name} must live on a GPU (cuda/hip device), got {t.device}")
    if device is not None and t.device != device:
        raise ValueError(f"{name} is on {t.device}, expected {device}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if tuple(t.shape[1:]) != tuple(shape_tail):
        raise ValueError(f"{name} must have shape (*, {', '.join(map(str, shape_tail))}), got {tuple(t.shape)}")


def _validate(pointcloud, features, mask, obj, q, t, camera_info):
    """Checks the tensors of a GaussianPointCloudRasterisationInput; returns the intrinsics as the kernels read them."""
    dev = pointcloud.device
    _require(pointcloud, "point_cloud", torch.float32, (3,))
    _require(features, "point_cloud_features", torch.float32, (56,), dev)
    if features.shape[0] != pointcloud.shape[0] or mask.shape[0] != pointcloud.shape[0] or obj.shape[0] != pointcloud.shape[0]:
        raise ValueError("point_cloud, point_cloud_features, point_invalid_mask and point_object_id disagree on N")
    _require(mask, "point_invalid_mask", torch.int8, (), dev)
    _require(obj, "point_object_id", torch.int32, (), dev)
    _require(q, "q_pointcloud_camera", torch.float32, (4,), dev)
    _require(t, "t_pointcloud_camera", torch.float32, (3,), dev)
    if q.shape[0] != t.shape[0] or q.shape[0] < 1:
        raise ValueError("q_pointcloud_camera and t_pointcloud_camera must have the same, non-zero number of rows")
    Kmat = camera_info.camera_intrinsics
    if tuple(Kmat.shape) != (3, 3):
        raise ValueError("camera_intrinsics must be 3x3")
    if Kmat.dtype != torch.float32 or Kmat.device != dev or not Kmat.is_contiguous():
        Kmat = Kmat.to(device=dev, dtype=torch.float32).contiguous()
    return Kmat


def _marshal(config, pointcloud, features, mask, obj, q, t, camera_info):
    """-> (gs_scene, gs_camera, gs_config, intrinsics) of validated inputs; the caller keeps the intrinsics tensor alive for as
    long as a kernel may read it (it is a fresh tensor when camera_info's had to be converted)."""
    Kmat = _validate(pointcloud, features, mask, obj, q, t, camera_info)
    return (_native.GsScene.of(pointcloud, features, mask, obj), _native.GsCamera.of(camera_info, q, t, Kmat),
            _native.GsConfig.of(config), Kmat)


def _marshal_input(config, inp):
    """_marshal of a GaussianPointCloudRasterisationInput"""
    return _marshal(config, inp.point_cloud, inp.point_cloud_features, inp.point_invalid_mask, inp.point_object_id,
                    inp.q_pointcloud_camera, inp.t_pointcloud_camera, inp.camera_info)


class _Contexts(dict):
    """device index -> _native.Context: the gs_ctx's of one operator instance, each created on first use."""

    def of(self, device: torch.device) -> "_native.Context":
        idx = _native.device_index(device)
        if idx not in self:
            self[idx] = _native.Context(idx)
        return self[idx]


class _Frame:
    """Owner of a gs_frame ticket: what ctx.save_for_backward keeps in the reference (RAST:998-1021).  Holds the
    context alive (the ticket is meaningless without it) and gives the ticket back when it dies."""

    def __init__(self, context: "_native.Context", handle, device, owned=True, lazy=False):
        """lazy: the frame was only begun (gs_project_shard_begin); its counts are read -- which waits for its kernels -- the
        first time one of them is asked for."""
        self._context, self._h, self.device, self._owned = context, handle, device, owned
        self.marshalled = None              # (gs_scene, gs_camera, gs_config) of the forward that made the frame
        if not lazy:
            self._read_info()

    @classmethod
    def of_call(cls, name, context, device, *args, keep, lazy=False):
        """The frame a forward-type library call makes: `name`(ctx, *args, keep_for_backward, &frame, stream)."""
        handle = _native.frame_out()
        _native.call(name, device, context.handle, *args, 1 if keep else 0, handle)
        return cls(context, handle, device, owned=keep, lazy=lazy)

    def _read_info(self):
        info = _native.GsFrameInfo()
        _native.call("gs_frame_get_info", self.device, self._context.handle, self.handle, info)
        self.n_points, self.n_points_in_camera, self.n_keys = info.n_points, info.n_points_in_camera, info.n_keys
        self.n_tiles, self.sort_key_bits, self.stages = info.n_tiles, info.sort_key_bits, info.stages
        self.sizing = ("exact", "predicted", "redone")[info.sizing]      # gs_frame_info.sizing: how the per-pixel half was sized

    def __getattr__(self, name):            # only reached for attributes not set yet: the counts of a lazy frame
        if name in ("n_points", "n_points_in_camera", "n_keys", "n_tiles", "sort_key_bits", "stages", "sizing"):
            self._read_info()
            return self.__dict__[name]
        raise AttributeError(name)

    @property
    def handle(self):
        if self._h is None:
            raise RuntimeError("frame already released")
        return self._h

    def export(self, name: str) -> torch.Tensor:
        eid, dtype, tail = _native.EXPORTS[name]
        with _native.on_device(self.device):    # a count, not a status: the one library call made beside _native.call()
            n = _native.lib().gs_frame_export_count(self._context.handle, self.handle, eid)
        if n < 0:
            raise RuntimeError(f"gs_frame_export_count({name}) failed: the frame is no longer live or does not hold that stage")
        rows = n
        for d in tail:
            rows //= d
        out = torch.empty((rows, *tail), dtype=_TORCH_DTYPES[dtype], device=self.device)
        if n > 0:
            _native.call("gs_frame_export", self.device, self._context.handle, self.handle, eid, _native.ptr(out),
                         what=f"gs_frame_export({name})")
        return out

    def heavy_tiles(self, items: bool = False) -> int:
        """Diagnostic: tiles the last backward blend of this frame shared among four waves, or (items=True) the work items they were
        handed out as -- one per 512-entry segment of a list the forward cut (gs_frame_heavy_tiles)."""
        n = _native.int32_pair()
        _native.call("gs_frame_heavy_tiles", self.device, self._context.handle, self.handle, n)
        return int(n[1] if items else n[0])

    def release(self):
        """Hands the ticket back.  Transient frames (forward without gradient tracking) belong to the context and are
        recycled by its next forward; their ticket then simply stops resolving."""
        h, self._h = self._h, None
        if h is not None:
            self._stale = h                 # the spent ticket: the library refuses it by itself (channels.py passes it on)
        if h is not None and self._owned and self._context.handle:
            _native.call("gs_frame_release", None, self._context.handle, h)

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass
