"""The float64 reference of the target resampler (include/gs_targets.h): ATen's _upsample_bilinear2d_aa with
align_corners=False -- torchvision's resize(antialias=True) on a float tensor -- restated in numpy, for down-scaling.
Per axis, with scale = in / out >= 1, support = scale and center = scale (i + 0.5), output i reads the inputs
[max(int(center - support + 0.5), 0), min(int(center + support + 0.5), in)) with the weights max(0, 1 - |(j - center + 0.5) / scale|)
divided by their sum; the horizontal pass runs first, then the vertical one.  No torch, no package import."""
import numpy as np


def axis_windows(n_in, n_out):
    """-> list of (first input, float64 weights) per output of one axis"""
    if not 1 <= n_out <= n_in:
        raise ValueError("down-scaling only: 1 <= out <= in")
    scale = n_in / n_out
    support = scale
    out = []
    for i in range(n_out):
        center = scale * (i + 0.5)
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), n_in)
        j = np.arange(lo, hi, dtype=np.float64)
        w = np.maximum(0.0, 1.0 - np.abs((j - center + 0.5) / scale))
        out.append((lo, w / w.sum()))
    return out


def axis_matrix(n_in, n_out, rows=None):
    """the (rows or n_out, n_in) float64 matrix of one axis: the first `rows` outputs"""
    windows = axis_windows(n_in, n_out)
    rows = n_out if rows is None else rows
    m = np.zeros((rows, n_in), np.float64)
    for i in range(rows):
        lo, w = windows[i]
        m[i, lo:lo + len(w)] = w
    return m


def resize_antialias(image_chw, size, crop=None):
    """image_chw (C,H,W) float64 -> the top-left `crop` (default: all) of its antialiased resize to `size`, float64"""
    image = np.asarray(image_chw, np.float64)
    h_full, w_full = size
    h, w = (h_full, w_full) if crop is None else crop
    mx = axis_matrix(image.shape[2], w_full, w)
    my = axis_matrix(image.shape[1], h_full, h)
    horizontal = image @ mx.T                    # (C,H,w)
    return my @ horizontal                       # (h,H) @ (C,H,w) -> (C,h,w)


def to_float(image_hwc_u8):
    """torchvision's to_tensor in float64 on the first three channels: (H,W,C) uint8 -> (3,H,W) of v / 255"""
    return np.asarray(image_hwc_u8)[..., :3].astype(np.float64).transpose(2, 0, 1) / 255.0


def target(image_hwc_u8, factor):
    """_downsample_image_and_camera_info's image (GaussianPointTrainer.py:103-109) of an (H,W,C) uint8 image, float64: the
    resize to (H // f, W // f), cropped to multiples of 16"""
    H, W = image_hwc_u8.shape[:2]
    h_full, w_full = H // factor, W // factor
    return resize_antialias(to_float(image_hwc_u8), (h_full, w_full), (h_full - h_full % 16, w_full - w_full % 16))
