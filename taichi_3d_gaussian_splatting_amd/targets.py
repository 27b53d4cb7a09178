"""Training targets on the device (include/gs_targets.h, csrc/k_targets.hip).

image_resample() is the library call: the top-left crop of the antialiased bilinear down-resize of a resident image --
torchvision's resize(antialias=True) on a float tensor, i.e. ATen's _upsample_bilinear2d_aa -- from uint8 HWC (any row pitch)
or f32 CHW to f32 CHW, in one launch.  TargetStore keeps a dataset's images on the device as the uint8 they were decoded to
and hands out, per step, what the reference trainer makes on the host from a DataLoader item
(GaussianPointTrainer.py:103-121, 149-159): the (3,h,w) f32 image at the current downsample factor, the pose and the
CameraInfo with its intrinsics divided by the factor.

There is no fallback path: every call goes through _native.call(), and a CPU tensor is refused.
"""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor
from typing import Optional, Tuple

import torch

from . import _native
from .Camera import CameraInfo

FORMAT_U8_HWC, FORMAT_F32_CHW = 0, 1
# the output tile of one workgroup (GS_RESAMPLE_TILE_H / _W in gs_targets.h) and the bounds of a call
TILE_H, TILE_W = 16, 64
MAX_SCALE = 8
MAX_SIZE = 32768
ROW_PITCH_ALIGN = 16            # bytes: rows of a stored image start on 16-byte boundaries (aligned 16-byte loads)
MAX_RESOLUTION_TRAIN = 1600     # ImagePoseDataset.py:13
MAX_DECODE_THREADS = 8

_VP, _I32, _I64 = C.c_void_p, C.c_int32, C.c_int64
ARGTYPES = {
    # (ctx, src, src_format, src_channels, H_in, W_in, src_row_pitch_bytes, h_full, w_full, h_out, w_out, dst, stream)
    "gs_image_resample": [_VP, _VP, _I32, _I32, _I32, _I32, _I64, _I32, _I32, _I32, _I32, _VP, _VP],
    # the same arguments; src_channels must be 4 and dst is (4, h_out, w_out) (include/gs_targets_rgba.h)
    "gs_image_resample_rgba": [_VP, _VP, _I32, _I32, _I32, _I32, _I64, _I32, _I32, _I32, _I32, _VP, _VP],
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


def _source_layout(src):
    """-> (format, channels, H, W, row pitch in bytes) of a source tensor, or ValueError"""
    if not isinstance(src, torch.Tensor) or src.dim() != 3:
        raise ValueError("the source must be a uint8 (H,W,C) or a float32 (C,H,W) tensor")
    if not src.is_cuda:
        raise ValueError(f"targets are resampled on the GPU: the source is on {src.device}, move it to a cuda/hip device first "
                         "(there is no CPU path)")
    if src.dtype == torch.uint8:
        H, W, ch = src.shape
        if ch not in (3, 4) or (W > 0 and H > 0 and (src.stride(2) != 1 or src.stride(1) != ch or (H > 1 and src.stride(0) < W * ch))):
            raise ValueError("a uint8 source must be (H,W,3) or (H,W,4) with dense pixels and a row stride >= W*C")
        return FORMAT_U8_HWC, ch, H, W, (src.stride(0) if H > 1 else W * ch)
    if src.dtype == torch.float32:
        ch, H, W = src.shape
        if ch not in (3, 4) or not src.is_contiguous():
            raise ValueError("a float32 source must be a contiguous (3,H,W) or (4,H,W) tensor")
        return FORMAT_F32_CHW, ch, H, W, W * 4
    raise ValueError(f"the source must be uint8 or float32, got {src.dtype}")


def image_resample(src: torch.Tensor, size_full: Tuple[int, int], size_out: Optional[Tuple[int, int]] = None,
                   out: Optional[torch.Tensor] = None, alpha: bool = False) -> torch.Tensor:
    """-> (3, h_out, w_out) f32: the top-left size_out crop (default: all) of the antialiased resize of src to size_full.
    src: uint8 (H,W,3|4) with any row stride, or contiguous f32 (3|4,H,W); channel 3 is ignored.  The scale H / h_full and
    W / w_full must be in [1, 8].  Queued on the current stream of the source's device; no host synchronisation.  out: the tensor
    to write (contiguous f32 (3,h_out,w_out) on the same device); a new one otherwise.
    alpha=True (gs_image_resample_rgba): the source must have four channels, and the result is (4, h_out, w_out): planes 0..2
    as without it, bit for bit, plane 3 channel 3 through the same filter -- the per-pixel weight of the target, same launch."""
    _bind()
    fmt, ch, H, W, pitch = _source_layout(src)
    planes, entry = (4, "gs_image_resample_rgba") if alpha else (3, "gs_image_resample")
    if alpha and ch != 4:
        raise ValueError(f"alpha=True needs a four-channel source, got {ch} channels")
    h_full, w_full = int(size_full[0]), int(size_full[1])
    h_out, w_out = (h_full, w_full) if size_out is None else (int(size_out[0]), int(size_out[1]))
    if out is None:
        if min(h_out, w_out) < 0:
            raise ValueError("the output size must not be negative")
        out = torch.empty((planes, h_out, w_out), dtype=torch.float32, device=src.device)
    elif out.dtype != torch.float32 or out.device != src.device or tuple(out.shape) != (planes, h_out, w_out) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 ({planes},{h_out},{w_out}) tensor on {src.device}")
    _native.call(entry, src.device, _native.shared_ctx(src.device), _native.ptr(src), fmt, ch, H, W, pitch,
                 h_full, w_full, h_out, w_out, _native.ptr(out))
    return out


def autoscale_size(height: int, width: int, size: int = 1024, max_size: int = MAX_RESOLUTION_TRAIN) -> Tuple[int, int]:
    """(h, w) of torchvision's resize(size=1024, max_size=1600): the short side to `size`, the long side capped at max_size"""
    short, long = (width, height) if width <= height else (height, width)
    new_short, new_long = size, int(size * long / short)
    if new_long > max_size:
        new_short, new_long = int(max_size * new_short / new_long), max_size
    return (new_long, new_short) if width <= height else (new_short, new_long)


def downsampled_geometry(height: int, width: int, downsample_factor: int) -> Tuple[int, int, int, int]:
    """-> (h_full, w_full, h, w) of _downsample_image_and_camera_info (GaussianPointTrainer.py:104-108): the resize to
    (H // f, W // f) and its crop to multiples of 16"""
    h_full, w_full = height // downsample_factor, width // downsample_factor
    return h_full, w_full, h_full - h_full % 16, w_full - w_full % 16


def downsampled_intrinsics(camera_intrinsics: torch.Tensor, downsample_factor: int) -> torch.Tensor:
    """fx, fy, cx, cy divided by the factor (GaussianPointTrainer.py:110-115); (3,3) or (n,3,3), a new tensor"""
    k = camera_intrinsics.clone()
    k[..., 0, 0] /= downsample_factor
    k[..., 1, 1] /= downsample_factor
    k[..., 0, 2] /= downsample_factor
    k[..., 1, 2] /= downsample_factor
    return k


def scaled_intrinsics(camera_intrinsics: torch.Tensor, scale_x: float, scale_y: float) -> torch.Tensor:
    """fx, cx times scale_x and fy, cy times scale_y (the autoscale of ImagePoseDataset.py:46-56); a new (3,3) tensor"""
    k = camera_intrinsics.clone()
    k[0, 0] *= scale_x
    k[1, 1] *= scale_y
    k[0, 2] *= scale_x
    k[1, 2] *= scale_y
    return k


def autoscaled_camera_info(camera_info: CameraInfo):
    """-> ((h_full, w_full) of the autoscale resize, the CameraInfo behind it: cropped to multiples of 16, intrinsics scaled by
    resized / original size), or (None, camera_info) for an image within MAX_RESOLUTION_TRAIN"""
    H, W = int(camera_info.camera_height), int(camera_info.camera_width)
    if H <= MAX_RESOLUTION_TRAIN and W <= MAX_RESOLUTION_TRAIN:
        return None, camera_info
    h_full, w_full = autoscale_size(H, W)
    return (h_full, w_full), CameraInfo(camera_intrinsics=scaled_intrinsics(camera_info.camera_intrinsics, w_full / W, h_full / H),
                                        camera_height=h_full - h_full % 16, camera_width=w_full - w_full % 16,
                                        camera_id=camera_info.camera_id)


def erode_mask(mask_hw: torch.Tensor, k: int) -> torch.Tensor:
    """a uint8 (H,W) mask shrunk by k pixels: a pixel keeps the minimum of its (2k+1) x (2k+1) neighbourhood (what lies outside
    the image does not shrink it).  Plain torch, once at load."""
    k = int(k)
    if k <= 0:
        return mask_hw
    inv = 255.0 - mask_hw.to(torch.float32)[None, None]
    grown = torch.nn.functional.max_pool2d(inv, kernel_size=2 * k + 1, stride=1, padding=k)      # pads with -inf
    return (255.0 - grown[0, 0]).to(torch.uint8)


def _with_mask(image_hwc: torch.Tensor, mask_hw: torch.Tensor) -> torch.Tensor:
    """(H,W,4) uint8: channels 0..2 of the image, the mask as channel 3"""
    H, W = image_hwc.shape[0], image_hwc.shape[1]
    if mask_hw.dtype != torch.uint8 or tuple(mask_hw.shape) != (H, W):
        raise ValueError(f"a mask must be uint8 ({H},{W}), the picture's size; got {mask_hw.dtype} {tuple(mask_hw.shape)}")
    return torch.cat([image_hwc[:, :, :3], mask_hw[:, :, None]], dim=2).contiguous()


def _pitched(image, device) -> torch.Tensor:
    """a (H,W) or (H,W,C) uint8 or uint16 CPU tensor or array on the device, rows ROW_PITCH_ALIGN-byte aligned: a view into a
    (H, pitch) buffer"""
    image = torch.as_tensor(image).contiguous()
    H, row = image.shape[0], image[0].numel()
    align = ROW_PITCH_ALIGN // image.element_size()
    pitch = (row + align - 1) // align * align
    host = torch.zeros((H, pitch), dtype=image.dtype)
    host[:, :row] = image.reshape(H, row)
    return host.to(device).as_strided(image.shape, (pitch,) + image.stride()[1:])


class ResidentStore:
    """What the stores of a dataset's per-view data resident on one device share (TargetStore here, depth.DepthStore,
    geometry.NormalStore): `records`, one device tensor per view or None, and `sizes`, the (H, W) of the dataset's crop of each
    picture.  A store adds what a decoded record becomes on the device (from_dataset) and a target() that fills the buffer of
    _buffer() from _source() with its resample call."""
    column = holds = ""                             # the dataset column and what a record holds, for the messages

    def __init__(self, records, sizes, device):
        self.device = self.on_gpu(device)
        self.records, self.sizes = list(records), list(sizes)
        self._outs = {}                             # planes -> {(H, W, factor) -> the (planes,h,w) buffer of that geometry}

    @classmethod
    def on_gpu(cls, device) -> torch.device:
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"a {cls.__name__} lives on a GPU, got {device} (there is no CPU path)")
        return device

    def __len__(self):
        return len(self.records)

    def has(self, i: int) -> bool:
        return self.records[i] is not None

    @classmethod
    def _decode(cls, loader, n: int, require_all: bool = True) -> list:
        """-> [loader(i) for i < n], decoded once in this process (no worker processes: the GPU may be initialised).
        require_all: a record the loader has nothing for is an error (False: it stays None)"""
        with ThreadPoolExecutor(max_workers=max(1, min(MAX_DECODE_THREADS, n))) as pool:
            loaded = list(pool.map(loader, range(n)))
        missing = [i for i, item in enumerate(loaded) if item is None]
        if require_all and missing:
            raise ValueError(f"record {missing[0]} of the dataset has no {cls.column}")
        return loaded

    def _source(self, i: int) -> torch.Tensor:
        """what the resample call reads of view i: an integer-typed record is stored uncropped, the dataset's crop is its
        top-left region"""
        src, (H, W) = self.records[i], self.sizes[i]
        return src if src.dtype.is_floating_point else src[:H, :W]

    def _buffer(self, i: int, downsample_factor: int, planes: int):
        """-> ((h_full, w_full), (h, w), out): downsampled_geometry of view i at the factor and the store's (planes,h,w) f32
        buffer of that geometry, allocated at its first use"""
        f = int(downsample_factor)
        if f < 1:
            raise ValueError(f"downsample_factor must be >= 1, got {downsample_factor}")
        if self.records[i] is None:
            raise ValueError(f"view {i} has no {self.holds}")
        H, W = self.sizes[i]
        h_full, w_full, h, w = downsampled_geometry(H, W, f)
        outs = self._outs.setdefault(planes, {})
        out = outs.get((H, W, f))
        if out is None:
            out = outs[(H, W, f)] = torch.empty((planes, h, w), dtype=torch.float32, device=self.device)
        return (h_full, w_full), (h, w), out


class TargetStore(ResidentStore):
    """The images of a dataset resident on one device, and the per-step target made from them there.

    from_dataset() decodes every image once, in this process (no worker processes: the GPU may be initialised), and keeps
      - the image as uint8 (H,W,C) with 16-byte aligned rows, uncropped: the dataset's crop to multiples of 16 is the top-left
        region the kernel reads; or, for an image over MAX_RESOLUTION_TRAIN, its autoscaled version (resize(size=1024,
        max_size=1600) of the cropped image, ImagePoseDataset.py:41-62) as f32 (3,h,w), made once by the same kernel;
      - q (n,4), t (n,3) and the intrinsics (n,3,3) as device tensors, and the base CameraInfo of every view.
    With mask_source ("alpha": the RGBA image's own alpha; "file": the dataset's mask_path image, packed into channel 3 at load)
    every stored image has four channels, and target(i, f, with_weight=True) also returns the mask through the same filter.
    target(i, f) then costs one launch.  The image it returns is the store's buffer for that geometry and is overwritten by the
    next target() of the same geometry: use it (loss forward and backward) before asking for the next one."""
    column = "image_path"

    def __init__(self, images, q: torch.Tensor, t: torch.Tensor, camera_infos, device):
        camera_infos = list(camera_infos)
        super().__init__(images, [(int(c.camera_height), int(c.camera_width)) for c in camera_infos], device)
        self.images = self.records
        self.q, self.t = q.to(self.device), t.to(self.device)
        self.intrinsics = {1: torch.stack([c.camera_intrinsics.to(torch.float32) for c in camera_infos]).to(self.device)}
        # intrinsics on the device: views of self.intrinsics[1]
        self.camera_infos = [CameraInfo(camera_intrinsics=self.intrinsics[1][i], camera_height=int(c.camera_height),
                                        camera_width=int(c.camera_width), camera_id=c.camera_id) for i, c in enumerate(camera_infos)]
        self._infos = {}                            # (view, factor) -> CameraInfo

    @property
    def _out(self):
        """the (3,h,w) buffers handed out so far, by geometry"""
        return self._outs.get(3, {})

    @classmethod
    def from_dataset(cls, dataset, device="cuda", mask_source: Optional[str] = None, mask_erode: int = 0) -> "TargetStore":
        """mask_source None: as ever.  "alpha": every image must decode to RGBA; its alpha is the weight.  "file": every record
        must have a mask_path (dataset.load_mask); the mask replaces channel 3.  mask_erode=k shrinks the mask by k pixels
        first (k = 5: no 11-tap SSIM window with a weight sees a masked pixel)."""
        if mask_source not in (None, "alpha", "file"):
            raise ValueError(f'mask_source must be None, "alpha" or "file", got {mask_source!r}')
        if int(mask_erode) < 0 or (mask_source is None and int(mask_erode) != 0):
            raise ValueError("mask_erode must be >= 0, and needs a mask_source")
        device = torch.device(device)
        n = len(dataset)
        raw = cls._decode(dataset.load_raw, n)
        masks = cls._decode(dataset.load_mask, n, require_all=False) if mask_source == "file" else [None] * n
        images, qs, ts, infos = [], [], [], []
        for i, (image_hwc, q, t, info) in enumerate(raw):
            if mask_source == "file":
                if masks[i] is None:
                    raise ValueError(f'mask_source="file": record {i} of the dataset has no mask_path')
                mask = masks[i] if isinstance(masks[i], torch.Tensor) else torch.from_numpy(masks[i])
                image_hwc = _with_mask(image_hwc, erode_mask(mask, mask_erode))
            elif mask_source == "alpha":
                if image_hwc.shape[2] != 4:
                    raise ValueError(f'mask_source="alpha": image {i} of the dataset has no alpha channel')
                if mask_erode:
                    image_hwc = _with_mask(image_hwc, erode_mask(image_hwc[:, :, 3], mask_erode))
            stored = _pitched(image_hwc, device)
            H, W = int(info.camera_height), int(info.camera_width)          # the dataset's crop of the decoded image
            size_full, info = autoscaled_camera_info(info)
            if size_full is not None:
                stored = image_resample(stored[:H, :W], size_full, (info.camera_height, info.camera_width), alpha=mask_source is not None)
            images.append(stored)
            qs.append(q.reshape(4))
            ts.append(t.reshape(3))
            infos.append(info)
        return cls(images, torch.stack(qs).to(torch.float32), torch.stack(ts).to(torch.float32), infos, device)

    def target(self, i: int, downsample_factor: int = 1, with_weight: bool = False):
        """-> (image (3,h,w) f32, q (1,4), t (1,3), CameraInfo) of view i at the factor: sizes and intrinsics as
        _downsample_image_and_camera_info has them; at factor 1 the dataset's own crop.  After the first use of a geometry
        (image size, factor) the call allocates nothing on the device, copies nothing to it and does not synchronise.
        with_weight=True (the stored image must have four channels): -> (image, q, t, CameraInfo, weight (h,w) f32); image and
        weight are out[:3] and out[3] of one (4,h,w) buffer, both contiguous, written by one launch; the image is bit for bit
        the one target(i, f) returns."""
        size_full, (h, w), out = self._buffer(i, downsample_factor, 4 if with_weight else 3)
        f = int(downsample_factor)
        if f not in self.intrinsics:
            self.intrinsics[f] = downsampled_intrinsics(self.intrinsics[1], f)
        info = self._infos.get((i, f))
        if info is None:
            info = self._infos[(i, f)] = CameraInfo(camera_intrinsics=self.intrinsics[f][i], camera_height=h, camera_width=w,
                                                    camera_id=self.camera_infos[i].camera_id)
        image_resample(self._source(i), size_full, (h, w), out=out, alpha=with_weight)
        if with_weight:
            return out[:3], self.q[i:i + 1], self.t[i:i + 1], info, out[3]
        return out, self.q[i:i + 1], self.t[i:i + 1], info
