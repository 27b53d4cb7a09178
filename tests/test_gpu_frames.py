"""GPU: the 8-bit frame conversion (k_frames.hip through frames.py) bit for bit against the torch CPU expressions it replaces,
the exact sum of squared differences against numpy's, and the FrameSink's ring."""
import os

import numpy as np
import pytest
import torch

from taichi_3d_gaussian_splatting_amd import frames

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(1, 1), (16, 16), (17, 23), (48, 64)]


def _neighbours(v):
    v = np.asarray(v, np.float32)
    return np.concatenate([v, np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))])


def rgb_values():
    """every k/255 and its two f32 neighbours, the same for the rounding thresholds (k + 0.5)/255, +-0, negatives, values
    above 1, +-inf, denormals -- and NaN, which the torch expression does not define and the kernel maps to 0"""
    k = np.arange(256, dtype=np.float32)
    special = np.array([0.0, -0.0, -1e-3, -1.0, -1e30, 1.0000001, 1.5, 2.0, 1e30, np.inf, -np.inf, 1e-45, -1e-45, 1e-39, 1.1754942e-38,
                        0.00392, 0.99999994, 3.4e38, -3.4e38], np.float32)
    return np.concatenate([_neighbours(k / np.float32(255.0)), _neighbours((k + np.float32(0.5)) / np.float32(255.0)), special,
                           np.array([np.nan], np.float32)])


def depth_values():
    """the depths at which a channel of the colour map crosses k/255 (and their neighbours), its three ranges' ends, and the
    specials above"""
    k = np.arange(256, dtype=np.float32) / np.float32(255.0)
    cross = np.concatenate([10 * (1 - k), 10 + 50 * (1 - k), 60 + 200 * (1 - k)]).astype(np.float32)
    ends = np.array([0.0, -0.0, 10.0, 60.0, 260.0, -1.0, 1e-45, 1e30, np.inf, -np.inf, 0.8, 1000.0], np.float32)
    return np.concatenate([_neighbours(cross), _neighbours(ends), np.array([np.nan], np.float32)])


def _tiled(values, count, offset):
    idx = (np.arange(count) * 7 + offset) % values.size
    return values[idx]


def reference(src, mode):
    """the torch CPU expression of each mode; src a CPU tensor without NaN"""
    if mode == frames.RGB_TRUNC:
        return torch.clamp(src * 255, 0, 255).byte()
    if mode == frames.RGB_ROUND:
        return torch.clamp(torch.floor(src * 255 + 0.5), 0, 255).byte()
    x_rgb = torch.zeros((3, src.shape[0], src.shape[1]), dtype=torch.float32)
    x_rgb[0] = torch.clamp(src, 0, 10) / 10.
    x_rgb[1] = torch.clamp(src - 10, 0, 50) / 50.
    x_rgb[2] = torch.clamp(src - 60, 0, 200) / 200.
    image = (1. - x_rgb).permute(1, 2, 0)
    return torch.clamp(image * 255, 0, 255).byte()


def _out(h, w, extra):
    """an (h,w,3) uint8 view with row pitch 3w + extra in a buffer of 0xAB, and the buffer"""
    pitch = 3 * w + extra
    buf = torch.full((h * pitch + 16,), 0xAB, dtype=torch.uint8, device=DEV)
    return buf.as_strided((h, w, 3), (pitch, 3, 1)), buf, pitch


@pytest.mark.parametrize("extra", [0, 5])
@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("mode", [frames.RGB_TRUNC, frames.RGB_ROUND, frames.DEPTH_CMAP])
def test_bit_exact_against_torch(mode, h, w, extra):
    values = depth_values() if mode == frames.DEPTH_CMAP else rgb_values()
    shape = (h, w) if mode == frames.DEPTH_CMAP else (h, w, 3)
    count = int(np.prod(shape))
    for r in range(min(-(-values.size // count), 8)):           # the small sizes see a part of the list, the next test all of it
        src = torch.from_numpy(_tiled(values, count, 7 * r * count).reshape(shape).copy())
        nan = torch.isnan(src)
        want = reference(torch.where(nan, torch.zeros_like(src), src), mode)
        want[nan] = 0                                               # (h,w) indexes the pixels of a depth, (h,w,3) the values
        out, buf, pitch = _out(h, w, extra)
        got = frames.frame_to_u8(src.to(DEV), mode, out=out)
        assert torch.equal(got.cpu(), want), (mode, h, w, extra, r)
        raw = buf.cpu().numpy()
        rows = raw[:h * pitch].reshape(h, pitch)
        assert (rows[:, 3 * w:] == 0xAB).all() and (raw[h * pitch:] == 0xAB).all()      # nothing past a row's 3w bytes


def test_every_listed_value_is_converted_as_torch_does():
    """all values at once, as one long row (w = number of values): no value is left to the tiling above"""
    for mode, values in ((frames.RGB_TRUNC, rgb_values()), (frames.RGB_ROUND, rgb_values()), (frames.DEPTH_CMAP, depth_values())):
        v = values[~np.isnan(values)]
        if mode == frames.DEPTH_CMAP:
            src = torch.from_numpy(v.reshape(1, -1).copy())
        else:
            src = torch.from_numpy(np.repeat(v, 3).reshape(1, -1, 3).copy())
        got = frames.frame_to_u8(src.to(DEV), mode).cpu()
        assert torch.equal(got, reference(src, mode)), mode
    nan = torch.full((2, 5, 3), float("nan"))
    assert int(frames.frame_to_u8(nan.to(DEV), frames.RGB_TRUNC).max()) == 0
    assert int(frames.frame_to_u8(nan.to(DEV), frames.RGB_ROUND).max()) == 0
    assert int(frames.frame_to_u8(nan[..., 0].contiguous().to(DEV), frames.DEPTH_CMAP).max()) == 0


def test_default_output_is_contiguous_and_takes_the_vector_path():
    g = torch.Generator().manual_seed(3)
    src = torch.rand(48, 64, 3, generator=g) * 1.2 - 0.1
    assert torch.equal(frames.frame_to_u8(src.to(DEV)).cpu(), reference(src, frames.RGB_TRUNC))
    # a source that is not 16-byte aligned takes the scalar loads: same bytes
    flat = torch.zeros(48 * 64 * 3 + 1, device=DEV)
    flat[1:] = src.reshape(-1).to(DEV)
    assert torch.equal(frames.frame_to_u8(flat[1:].view(48, 64, 3)).cpu(), reference(src, frames.RGB_TRUNC))


@pytest.mark.parametrize("channels,gt_extra", [(3, 0), (3, 7), (4, 0), (4, 16)])
@pytest.mark.parametrize("h,w", SIZES)
def test_sse_equals_numpys_integer_sum(h, w, channels, gt_extra):
    g = torch.Generator().manual_seed(h * 100 + w + channels)
    src = torch.rand(h, w, 3, generator=g)
    H, W = h + 2, w + 3                                          # the ground truth is larger: its top-left h x w is read
    pitch = W * channels + gt_extra
    gt_buf = torch.randint(0, 256, (H * pitch,), dtype=torch.uint8, generator=g)
    gt = gt_buf.to(DEV).as_strided((H, W, channels), (pitch, channels, 1))
    sse = torch.full((1,), 5, dtype=torch.int64, device=DEV)    # the sum is ADDED to the word
    out = frames.frame_to_u8(src.to(DEV), frames.RGB_TRUNC, gt=gt, sse=sse)
    want_out = reference(src, frames.RGB_TRUNC)
    assert torch.equal(out.cpu(), want_out)
    gt_np = gt_buf.numpy().reshape(H, pitch)[:h, :w * channels].reshape(h, w, channels)[:, :, :3].astype(np.int64)
    assert int(sse.item()) == 5 + int(((want_out.numpy().astype(np.int64) - gt_np) ** 2).sum())


def test_sse_extremes():
    h, w = 48, 64
    zeros, ones = torch.zeros(h, w, 3, device=DEV), torch.ones(h, w, 3, device=DEV)
    gt0, gt255 = torch.zeros(h, w, 3, dtype=torch.uint8, device=DEV), torch.full((h, w, 3), 255, dtype=torch.uint8, device=DEV)
    for src, gt, want in ((zeros, gt255, h * w * 3 * 255 ** 2), (ones, gt0, h * w * 3 * 255 ** 2), (zeros, gt0, 0), (ones, gt255, 0)):
        sse = torch.zeros(1, dtype=torch.int64, device=DEV)
        frames.frame_to_u8(src, frames.RGB_TRUNC, gt=gt, sse=sse)
        assert int(sse.item()) == want
    # an image against its own bytes
    src = torch.rand(h, w, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    own = frames.frame_to_u8(src)
    sse = torch.zeros(1, dtype=torch.int64, device=DEV)
    frames.frame_to_u8(src, gt=own, sse=sse)
    assert int(sse.item()) == 0


def _decode(path, fmt):
    if fmt == "npy":
        return np.load(path)
    if fmt == "png":
        import PIL.Image
        with PIL.Image.open(path) as im:
            assert im.mode == "RGB"
            return np.array(im)
    raw = open(path, "rb").read()
    magic, size, maxval, data = raw.split(b"\n", 3)
    w, h = (int(v) for v in size.split())
    assert magic == b"P6" and maxval == b"255" and len(data) == h * w * 3
    return np.frombuffer(data, np.uint8).reshape(h, w, 3)


@pytest.mark.parametrize("fmt", ["png", "ppm", "npy"])
def test_sink_passes_40_frames_through_3_slots_in_order(fmt, tmp_path):
    h, w, n = 32, 48, 40
    g = torch.Generator().manual_seed(7)
    base = torch.rand(h, w, 3, generator=g)
    depth = torch.rand(h, w, generator=g) * 100
    images = [(base * (0.5 + i / n) + i / 255.0).contiguous() for i in range(n)]
    gt = reference(images[3], frames.RGB_TRUNC).to(DEV)
    seen = []
    sink = frames.FrameSink(str(tmp_path), fmt=fmt, slots=3, device=DEV, slot_filled=lambda i, a: seen.append(i))
    assert 1 <= sink.n_threads <= 8
    for i, image in enumerate(images):
        assert sink.submit(image.to(DEV), depth=depth.to(DEV) if i % 10 == 0 else None, gt=gt if i % 2 == 1 else None) == i
    sse = sink.close()
    assert sorted(seen) == list(range(n)) and sse.shape == (n,) and sse.dtype == torch.int64
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("frame_")) == [f"frame_{i:03}.{fmt}" for i in range(n)]
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("depth_")) == [f"depth_{i:03}.{fmt}" for i in range(0, n, 10)]
    for i, image in enumerate(images):
        want = reference(image, frames.RGB_TRUNC).numpy()
        assert np.array_equal(_decode(tmp_path / f"frame_{i:03}.{fmt}", fmt), want), i
        want_sse = int(((want.astype(np.int64) - gt.cpu().numpy().astype(np.int64)) ** 2).sum()) if i % 2 == 1 else 0
        assert int(sse[i]) == want_sse, i
    assert int(sse[3]) == 0
    assert np.array_equal(_decode(tmp_path / f"depth_010.{fmt}", fmt), reference(depth, frames.DEPTH_CMAP).numpy())
    with pytest.raises(RuntimeError, match="close"):
        sink.submit(images[0].to(DEV))


def test_sink_without_a_directory_and_a_failing_writer(tmp_path):
    got = {}
    sink = frames.FrameSink(None, slots=2, device=DEV, slot_filled=lambda i, a: got.__setitem__(i, a[0].copy()))
    src = torch.rand(16, 16, 3, generator=torch.Generator().manual_seed(2))
    for _ in range(5):
        sink.submit(src.to(DEV))
    sink.close()
    assert sorted(got) == list(range(5)) and all(np.array_equal(a, reference(src, frames.RGB_TRUNC).numpy()) for a in got.values())

    def boom(i, a):
        raise OSError("disk full")
    sink = frames.FrameSink(None, slots=2, device=DEV, slot_filled=boom)
    sink.submit(src.to(DEV))
    with pytest.raises(OSError, match="disk full"):
        sink.close()
