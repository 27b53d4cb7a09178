"""Frames out of the device (include/gs_frames.h, csrc/k_frames.hip).

frame_to_u8() is the library call: an f32 (h,w,3) image or (h,w) depth becomes the uint8 (h,w,3) image that is written to a
file -- torch.clamp(image * 255, 0, 255).byte() of the reference renderer, bit for bit, in one launch -- and, against resident
ground-truth bytes, adds the exact sum of squared 8-bit differences to a device word.  FrameSink is what a render loop hands
its frames to: a ring of pinned host slots, the conversion on the caller's stream, the copy of the bytes (a quarter of the f32
frame) on a side stream, and a bounded pool of threads that encode each slot once its copy is done.

There is no fallback path: every conversion goes through _native.call(), and a CPU tensor is refused.
"""
import ctypes as C
import os
import threading
from concurrent.futures import ThreadPoolExecutor
from typing import Optional

import numpy as np
import torch

from . import _native

RGB_TRUNC, RGB_ROUND, DEPTH_CMAP = 0, 1, 2      # GS_FRAME_RGB_TRUNC, GS_FRAME_RGB_ROUND, GS_FRAME_DEPTH_CMAP
MAX_SIZE = 32768                                # GS_FRAME_MAX_SIZE
BYTES_PER_THREAD = 16                           # GS_FRAME_BYTES_PER_THREAD
MAX_WRITER_THREADS = 8
FORMATS = ("png", "ppm", "npy")

_VP, _I32, _I64 = C.c_void_p, C.c_int32, C.c_int64
ARGTYPES = {
    # (ctx, src, mode, h, w, dst, dst_row_pitch_bytes, gt, gt_channels, gt_row_pitch_bytes, sse, stream)
    "gs_frame_to_u8": [_VP, _VP, _I32, _I32, _I32, _VP, _I64, _VP, _I32, _I64, _VP, _VP],
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


def _gt_layout(gt, h, w, device):
    """-> (pointer, channels, row pitch in bytes) of resident ground-truth bytes: uint8 (>= h, >= w, 3|4), dense pixels"""
    if not isinstance(gt, torch.Tensor) or gt.dtype != torch.uint8 or gt.dim() != 3 or gt.device != device:
        raise ValueError(f"the ground truth must be a uint8 (H,W,3|4) tensor on {device}")
    H, W, ch = gt.shape
    if ch not in (3, 4) or H < h or W < w or gt.stride(2) != 1 or gt.stride(1) != ch or (H > 1 and gt.stride(0) < W * ch):
        raise ValueError(f"the ground truth must be (>= {h}, >= {w}, 3|4) with dense pixels and a row stride >= W*C")
    return _native.ptr(gt), ch, (gt.stride(0) if H > 1 else W * ch)


def frame_to_u8(src: torch.Tensor, mode: int = RGB_TRUNC, out: Optional[torch.Tensor] = None, gt: Optional[torch.Tensor] = None,
                sse: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> uint8 (h,w,3).  src: contiguous f32 (h,w,3) on a GPU (RGB_TRUNC: the reference's clamp(image * 255, 0, 255).byte();
    RGB_ROUND: floor(v * 255 + 0.5), clamped) or contiguous f32 (h,w) (DEPTH_CMAP: the trainer's _easy_cmap, then RGB_TRUNC).
    out: the uint8 (h,w,3) tensor to write, dense pixels, any row stride >= 3w; a new contiguous one otherwise.  gt with sse:
    resident ground-truth bytes, uint8 (>= h, >= w, 3|4) with any row stride, and a one-element int64 tensor to which the sum
    of (out - gt)^2 over the frame is ADDED (exact; zero it first).  Queued on the current stream; no host synchronisation."""
    _bind()
    if not isinstance(src, torch.Tensor) or not src.is_cuda:
        raise ValueError("frames are converted on the GPU: the source must be a tensor on a cuda/hip device (there is no CPU path)")
    if mode not in (RGB_TRUNC, RGB_ROUND, DEPTH_CMAP):
        raise ValueError(f"unknown mode {mode}")
    want = 2 if mode == DEPTH_CMAP else 3
    if src.dtype != torch.float32 or src.dim() != want or (want == 3 and src.shape[2] != 3) or not src.is_contiguous():
        raise ValueError("the source must be a contiguous float32 (h,w,3) image, or (h,w) depth for DEPTH_CMAP")
    h, w = int(src.shape[0]), int(src.shape[1])
    if out is None:
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=src.device)
    elif out.dtype != torch.uint8 or out.device != src.device or tuple(out.shape) != (h, w, 3) or \
            (h > 0 and w > 0 and (out.stride(2) != 1 or out.stride(1) != 3 or (h > 1 and out.stride(0) < 3 * w))):
        raise ValueError(f"out must be a uint8 ({h},{w},3) tensor on {src.device} with dense pixels and a row stride >= 3w")
    pitch = out.stride(0) if h > 1 and w > 0 else 3 * w
    gt_ptr, gt_channels, gt_pitch, sse_ptr = None, 0, 0, None
    if (gt is None) != (sse is None):
        raise ValueError("gt and sse go together")
    if gt is not None:
        if sse.dtype != torch.int64 or sse.numel() != 1 or sse.device != src.device:
            raise ValueError(f"sse must be a one-element int64 tensor on {src.device}")
        if h > 0 and w > 0:
            gt_ptr, gt_channels, gt_pitch = _gt_layout(gt, h, w, src.device)
            sse_ptr = sse.data_ptr()
    _native.call("gs_frame_to_u8", src.device, _native.shared_ctx(src.device), _native.ptr(src), mode, h, w, _native.ptr(out), pitch,
                 gt_ptr, gt_channels, gt_pitch, sse_ptr)
    return out


def psnr_from_sse(sse, n_values: int) -> np.ndarray:
    """8-bit PSNR in float64 from exact sums of squared byte differences over n_values bytes each: 10 log10(255^2 / mse);
    inf for identical images"""
    mse = np.asarray(sse, np.float64) / float(n_values)
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(255.0 ** 2 / mse)


def _write(path: str, fmt: str, array: np.ndarray):
    if fmt == "png":
        import PIL.Image
        PIL.Image.fromarray(array).save(path)
    elif fmt == "ppm":
        with open(path, "wb") as fh:
            fh.write(b"P6\n%d %d\n255\n" % (array.shape[1], array.shape[0]))
            fh.write(array.tobytes())
    else:
        np.save(path, array)


class FrameSink:
    """Where a render loop leaves its frames: submit() queues the 8-bit conversion on the current stream and the copy to a
    pinned host slot on a side stream, and returns at once; a pool of writer threads encodes each slot when its copy is done.

      sink = FrameSink(directory, fmt="png", slots=4)
      for ...: sink.submit(image, depth=depth, gt=stored_bytes)
      sse = sink.close()            # (frames,) int64 on the CPU: the exact SSE per frame against gt (0 where none was given)

    Frame i goes to <directory>/<prefix><i:03>.<fmt>, its depth map (with depth=) to <directory>/<depth_prefix><i:03>.<fmt>.
    directory None: nothing is written, the bytes still reach the host (slot_filled(i, array) is called if given).  A full ring
    blocks submit(): no frame is dropped, and a slot is reused only after its file is written.  The writers are min(8, CPUs)
    threads, never more than 16; an error in one of them is raised by the next submit() or by close()."""

    def __init__(self, directory: Optional[str], fmt: str = "png", slots: int = 4, prefix: str = "frame_", depth_prefix: str = "depth_",
                 device="cuda", slot_filled=None):
        if fmt not in FORMATS:
            raise ValueError(f"format must be one of {FORMATS}, got {fmt!r}")
        if slots < 1:
            raise ValueError("a FrameSink needs at least one slot")
        _bind()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"a FrameSink reads frames from a GPU, got {self.device} (there is no CPU path)")
        self.directory, self.fmt, self.prefix, self.depth_prefix = directory, fmt, prefix, depth_prefix
        if directory is not None:
            os.makedirs(directory, exist_ok=True)
        self.slots = slots
        self.slot_filled = slot_filled
        self.n_threads = max(1, min(MAX_WRITER_THREADS, os.cpu_count() or 1, 16))
        self._pool = ThreadPoolExecutor(max_workers=self.n_threads)
        self._free = [threading.Event() for _ in range(slots)]
        for e in self._free:
            e.set()
        self._pending = [None] * slots              # the future of the slot's writer
        self._host = [None] * slots                 # (2,h,w,3) pinned: colour and depth map
        self._dev = [None] * slots
        self._copy_stream = torch.cuda.Stream(device=self.device)
        self._sse = torch.zeros(256, dtype=torch.int64, device=self.device)
        self.count = 0
        self._closed = False

    def _slot_buffers(self, slot, h, w):
        if self._host[slot] is None or tuple(self._host[slot].shape[1:3]) != (h, w):
            self._host[slot] = torch.empty((2, h, w, 3), dtype=torch.uint8).pin_memory()
            self._dev[slot] = torch.empty((2, h, w, 3), dtype=torch.uint8, device=self.device)
        return self._host[slot], self._dev[slot]

    def _raise_writer_error(self, slot):
        fut, self._pending[slot] = self._pending[slot], None
        if fut is not None:
            fut.result()

    def submit(self, image: torch.Tensor, depth: Optional[torch.Tensor] = None, gt: Optional[torch.Tensor] = None,
               mode: int = RGB_TRUNC) -> int:
        """Queue frame number `count`: image f32 (h,w,3) (or uint8 (h,w,3|4) on the device, written as it is), optionally its
        (h,w) depth and the resident uint8 ground truth.  -> the frame's index.  Blocks only while every slot is waiting for
        its writer."""
        if self._closed:
            raise RuntimeError("submit() after close()")
        index = self.count
        slot = index % self.slots
        self._free[slot].wait()
        self._raise_writer_error(slot)
        h, w = int(image.shape[0]), int(image.shape[1])
        host, dev = self._slot_buffers(slot, h, w)
        if index >= self._sse.numel():              # on the same stream as the launches that wrote the old words
            self._sse = torch.cat([self._sse, torch.zeros_like(self._sse)])
        if image.dtype == torch.uint8:              # bytes that are resident already (a stored ground truth): copied, not converted
            if gt is not None:
                raise ValueError("a uint8 frame is written as it is; it takes no ground truth")
            dev[0].copy_(image[:, :, :3])
        else:
            frame_to_u8(image, mode, out=dev[0], gt=gt, sse=self._sse[index:index + 1] if gt is not None else None)
        parts = 1
        if depth is not None:
            frame_to_u8(depth, DEPTH_CMAP, out=dev[1])
            parts = 2
        current = torch.cuda.current_stream(self.device)
        converted = torch.cuda.Event()
        converted.record(current)
        self._copy_stream.wait_event(converted)
        with torch.cuda.stream(self._copy_stream):
            host[:parts].copy_(dev[:parts], non_blocking=True)
            copied = torch.cuda.Event()
            copied.record(self._copy_stream)
        self._free[slot].clear()
        self.count = index + 1
        self._pending[slot] = self._pool.submit(self._finish, slot, index, parts, copied)
        return index

    def _finish(self, slot, index, parts, copied):
        try:
            copied.synchronize()
            arrays = self._host[slot].numpy()
            if self.directory is not None:
                _write(os.path.join(self.directory, f"{self.prefix}{index:03}.{self.fmt}"), self.fmt, arrays[0])
                if parts == 2:
                    _write(os.path.join(self.directory, f"{self.depth_prefix}{index:03}.{self.fmt}"), self.fmt, arrays[1])
            if self.slot_filled is not None:
                self.slot_filled(index, arrays[:parts])
        finally:
            self._free[slot].set()

    def close(self) -> torch.Tensor:
        """Wait for every writer, raise the first error one of them met, -> the per-frame SSE, (count,) int64 on the CPU
        (the one read of the device words)."""
        if not self._closed:
            self._closed = True
            self._pool.shutdown(wait=True)
            for slot in range(self.slots):
                self._raise_writer_error(slot)
        return self._sse[:self.count].cpu()

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:
            self._closed = True
            self._pool.shutdown(wait=True)
        return False
