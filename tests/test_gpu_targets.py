"""GPU (-m gpu): gs_image_resample (include/gs_targets.h), raw and through targets.py, against the float64 restatement of
torchvision's antialiased resize (tests/resample_ref.py).

Tolerance, derived and not measured.  Samples lie in [0,1] and the weights of a window sum to 1, so every partial sum of a pass
lies in [0,1] and each fused multiply-add rounds by at most 2^-24 (half an ulp of 1 is 2^-25; 2^-24 leaves room for the
f32 rounding of the weight it multiplies by).  A pass over `taps` inputs therefore adds at most about (taps + 1) 2^-24: the
taps, and the rounding of the sample itself (v / 255, or the first pass's result).  A window holds taps <= 2 scale + 1 inputs.
  scale <= 4:  two passes of (9 + 1) 2^-24 = 1.2e-6, plus the f32 rounding of the weights (at most 2^-24 relative per weight,
               summing to 6e-8 per pass): ABS_TOL = 2e-6.
  scale  = 8:  2 (2 * 8 + 2) 2^-24 = 2.15e-6 plus the same margin: ABS_TOL_8 = 3e-6.
A case over its bound is a finding about the kernel, not a reason to widen the bound.

Cases: factors 1, 2, 4; a crop that ends before the resize does; a non-integer scale (windows of 2 and 3 taps); RGBA; the f32
CHW source; a uint8 tensor whose pitch (159 bytes) is neither 4- nor 16-aligned, with an output no 16-byte store can write;
an output past one workgroup tile in both axes and no multiple of it; scale 8 exactly and 8.5 refused; 1920x1088 at factor 4.
The first and last two rows and columns (truncated, renormalised windows) are checked on their own; factor 1 is bit-exact;
two runs are bit-identical; the words around the destination are left alone; TargetStore reuses its buffers."""
import functools

import numpy as np
import pytest
import torch

import resample_ref
from taichi_3d_gaussian_splatting_amd import targets
from taichi_3d_gaussian_splatting_amd.Camera import CameraInfo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ABS_TOL = 2e-6          # scale <= 4
ABS_TOL_8 = 3e-6        # scale 8
GUARD_BITS = 0x7FC12345  # a NaN with a payload: any write, and any read that reaches the output, shows


@functools.lru_cache(maxsize=None)
def pixels(H, W, C, seed=0):
    """a uint8 (H,W,C) image with structure at every scale: a gradient, stripes and noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([(x * 255) // max(W - 1, 1), (y * 255) // max(H - 1, 1), ((x // 3 + y // 5) % 2) * 255, (x + y) % 256][:C], axis=2)
    noise = rng.integers(0, 256, (H, W, C))
    out = np.where(rng.random((H, W, 1)) < 0.5, base, noise).astype(np.uint8)
    out.setflags(write=False)
    return out


def to_tensor(u8):
    """torchvision's to_tensor of an (H,W,C) uint8 array, on the device: u8.float().div(255) taken on the CPU, where to_tensor
    runs and div is the true division (on the device torch multiplies by the rounded reciprocal of a host scalar: 126 of the
    256 values come out one ulp away)"""
    return torch.from_numpy(np.array(u8)).permute(2, 0, 1)[:3].float().div(255).to(DEV)


def on_device(u8, pitch=None):
    """the image on the device as (H,W,C) uint8 with the given row pitch in bytes (default: dense)"""
    H, W, C = u8.shape
    pitch = W * C if pitch is None else pitch
    buf = torch.full((H * pitch + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    view = buf.as_strided((H, W, C), (pitch, C, 1))
    view.copy_(torch.from_numpy(np.array(u8)).to(DEV))
    return view


def guarded_out(h, w):
    """-> (buffer, view): a (3,h,w) destination inside a larger buffer of GUARD_BITS, two rows' worth of guard either side"""
    guard = 2 * max(w, 1) + 4            # a multiple of 4 words: the view stays 16-byte aligned when 3*h*w allows it
    guard += (-guard) % 4
    buf = torch.full((guard + 3 * h * w + guard,), GUARD_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    return buf, buf[guard:guard + 3 * h * w].view(3, h, w)


def check_guards(buf, h, w):
    words = buf.view(torch.int32)
    guard = (buf.numel() - 3 * h * w) // 2
    assert bool((words[:guard] == GUARD_BITS).all()) and bool((words[guard + 3 * h * w:] == GUARD_BITS).all()), "the kernel wrote outside its output"


def compare(got, want, tol):
    """the whole image and, separately, its first and last two rows and columns, whose windows are cut and renormalised"""
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == want.shape
    assert np.isfinite(got).all()
    err = np.abs(got - want)
    edges = {"rows 0-1": err[:, :2], "rows -2,-1": err[:, -2:], "columns 0-1": err[:, :, :2], "columns -2,-1": err[:, :, -2:]}
    for name, e in edges.items():
        assert e.max() <= tol, (name, float(e.max()))
    assert err.max() <= tol, float(err.max())


def run(src, size_full, size_out):
    buf, out = guarded_out(*size_out)
    got = targets.image_resample(src, size_full, size_out, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    check_guards(buf, *size_out)
    return out


@pytest.mark.parametrize("factor", [1, 2, 4])
def test_factors_on_rgb(factor):
    u8 = pixels(64, 96, 3)
    h_full, w_full, h, w = targets.downsampled_geometry(64, 96, factor)
    assert (h, w) == {1: (64, 96), 2: (32, 48), 4: (16, 16)}[factor]
    out = run(on_device(u8), (h_full, w_full), (h, w))
    compare(out, resample_ref.target(u8, factor), ABS_TOL)


def test_crop_ends_before_the_resize_does():
    u8 = pixels(80, 112, 3, seed=1)
    assert targets.downsampled_geometry(80, 112, 2) == (40, 56, 32, 48)
    out = run(on_device(u8), (40, 56), (32, 48))
    want = resample_ref.resize_antialias(resample_ref.to_float(u8), (40, 56))[:, :32, :48]     # the last row and column are interior ones
    compare(out, want, ABS_TOL)


def test_non_integer_scale():
    u8 = pixels(135, 240, 3, seed=2)
    counts = {len(w) for _, w in resample_ref.axis_windows(240, 200)}
    assert {2, 3} <= counts
    out = run(on_device(u8), (128, 200), (128, 192))
    compare(out, resample_ref.resize_antialias(resample_ref.to_float(u8), (128, 200), (128, 192)), ABS_TOL)


def test_rgba_source_ignores_alpha():
    u8 = pixels(64, 96, 4, seed=3)
    out = run(on_device(u8), (32, 48), (32, 48))
    compare(out, resample_ref.target(u8, 2), ABS_TOL)
    other = u8.copy()
    other[..., 3] = 255 - other[..., 3]
    assert torch.equal(run(on_device(other), (32, 48), (32, 48)), out)


@pytest.mark.parametrize("size_full,size_out", [((32, 48), (32, 48)), ((21, 30), (16, 16)), ((64, 96), (64, 96)), ((64, 96), (48, 80))])
def test_f32_chw_source(size_full, size_out):
    image = np.random.default_rng(4).uniform(0.0, 1.0, (3, 64, 96)).astype(np.float32)
    src = torch.from_numpy(image).to(DEV)
    out = run(src, size_full, size_out)
    if size_full == (64, 96):
        assert torch.equal(out, src[:, :size_out[0], :size_out[1]])  # equal sizes: the input, cropped, bit for bit
    compare(out, resample_ref.resize_antialias(image, size_full, size_out), ABS_TOL)


def test_external_tensor_with_an_odd_pitch():
    u8 = pixels(37, 53, 3, seed=5)
    src = on_device(u8, pitch=159)
    assert src.stride(0) == 159 and 159 % 4 != 0
    out = run(src, (9, 13), (9, 13))                               # scale 4.11 / 4.08; w_out = 13: no 16-byte store
    # 37 / 9 = 4.11: a window still holds at most 9 inputs, the count ABS_TOL is derived for
    assert max(len(w) for n_in, n_out in ((37, 9), (53, 13)) for _, w in resample_ref.axis_windows(n_in, n_out)) <= 9
    compare(out, resample_ref.resize_antialias(resample_ref.to_float(u8), (9, 13)), ABS_TOL)
    # and from an address that is not even 4-aligned
    shifted = torch.zeros(37 * 159 + 3, dtype=torch.uint8, device=DEV)[3:].as_strided((37, 53, 3), (159, 3, 1))
    assert shifted.data_ptr() % 4 == 3
    shifted.copy_(src)
    assert torch.equal(run(shifted, (9, 13), (9, 13)), out)


def test_output_past_one_tile_in_both_axes():
    h, w = targets.TILE_H + 5, 2 * targets.TILE_W + 3
    H, W = 2 * h + 1, 3 * w + 2
    u8 = pixels(H, W, 3, seed=6)
    out = run(on_device(u8, pitch=(W * 3 + 15) // 16 * 16), (h, w), (h, w))
    compare(out, resample_ref.resize_antialias(resample_ref.to_float(u8), (h, w)), ABS_TOL)
    # the same output cropped by one row and three columns: every value it keeps is the same bits
    cropped = run(on_device(u8), (h, w), (h - 1, w - 3))
    assert torch.equal(cropped, out[:, :h - 1, :w - 3])


def test_scale_eight_and_beyond():
    u8 = pixels(128, 192 + 9, 4, seed=7)
    src = on_device(u8)
    out = run(src[:, :192], (16, 24), (16, 16))                    # a column crop of the source: pitch > W * C
    want = resample_ref.resize_antialias(resample_ref.to_float(u8[:, :192]), (16, 24), (16, 16))
    assert 15 <= max(len(w) for _, w in resample_ref.axis_windows(128, 16)) <= 17      # 2 * 8 + 1 at the most
    compare(out, want, ABS_TOL_8)
    tall = on_device(pixels(136, 96, 3, seed=8))
    with pytest.raises(RuntimeError, match=r"scale .* \[1, 8\]"):
        targets.image_resample(tall, (16, 48))                     # 8.5
    with pytest.raises(RuntimeError, match="scale"):
        targets.image_resample(tall, (137, 96))                    # upscaling
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def full_hd():
    u8 = pixels(1088, 1920, 3, seed=9)
    return u8, on_device(u8, pitch=1920 * 3)


def test_full_hd_at_factor_four(full_hd):
    u8, src = full_hd
    assert targets.downsampled_geometry(1088, 1920, 4) == (272, 480, 272, 480)
    out = run(src, (272, 480), (272, 480))
    compare(out, resample_ref.target(u8, 4), ABS_TOL)


def test_factor_one_is_bit_exact_and_runs_repeat(full_hd):
    u8, src = full_hd
    out = run(src, (1088, 1920), (1088, 1920))
    assert torch.equal(out, to_tensor(u8))
    small = pixels(80, 112, 4, seed=10)
    dev = on_device(small, pitch=112 * 4 + 16)
    assert torch.equal(run(dev, (80, 112), (64, 96)), to_tensor(small)[:, :64, :96])
    a = run(src, (544, 960), (544, 960)).clone()
    b = run(src, (544, 960), (544, 960))
    assert torch.equal(a, b)


def test_empty_outputs_launch_nothing():
    src = on_device(pixels(64, 96, 3))
    assert tuple(targets.image_resample(src, (32, 48), (0, 48)).shape) == (3, 0, 48)
    assert tuple(targets.image_resample(src, (32, 48), (32, 0)).shape) == (3, 32, 0)
    torch.cuda.synchronize()


# ---- TargetStore ----------------------------------------------------------------------------------------------------------------
def store_of(images):
    n = len(images)
    infos = [CameraInfo(torch.tensor([[100.0 + i, 0.0, 56.0], [0.0, 90.0, 40.0], [0.0, 0.0, 1.0]]), im.shape[0] // 16 * 16,
                        im.shape[1] // 16 * 16, i) for i, im in enumerate(images)]
    stored = [targets._pitched(torch.from_numpy(np.array(im)), DEV) for im in images]
    q = torch.nn.functional.normalize(torch.arange(4.0 * n).reshape(n, 4) + 1.0, dim=1)
    return targets.TargetStore(stored, q, torch.arange(3.0 * n).reshape(n, 3), infos, DEV), q


def test_target_store_targets_and_camera_info():
    images = [pixels(80, 112, 3, seed=11), pixels(80, 112, 4, seed=12), pixels(87, 120, 3, seed=13)]
    store, q = store_of(images)
    assert len(store) == 3 and all(im.stride(0) % 16 == 0 for im in store.images)
    for i, u8 in enumerate(images):
        H, W = u8.shape[0] // 16 * 16, u8.shape[1] // 16 * 16
        for f in (1, 2, 4):
            image, qi, ti, info = store.target(i, f)
            want = resample_ref.target(u8[:H, :W], f)
            compare(image, want, ABS_TOL)
            assert (info.camera_height, info.camera_width, info.camera_id) == (want.shape[1], want.shape[2], i)
            k = torch.tensor([[(100.0 + i) / f, 0.0, 56.0 / f], [0.0, 90.0 / f, 40.0 / f], [0.0, 0.0, 1.0]])
            assert info.camera_intrinsics.is_cuda and torch.equal(info.camera_intrinsics.cpu(), k)
            assert tuple(qi.shape) == (1, 4) and tuple(ti.shape) == (1, 3) and torch.equal(qi.cpu()[0], q[i])
    image, _, _, _ = store.target(0, 1)
    assert torch.equal(image, to_tensor(images[0]))


def test_target_store_reuses_its_buffers():
    store, _ = store_of([pixels(80, 112, 3, seed=11), pixels(80, 112, 3, seed=14)])
    first, _, _, info_a = store.target(0, 2)
    kept = first.clone()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    second, _, _, info_b = store.target(1, 2)                      # the same geometry, another view
    again, _, _, info_c = store.target(0, 2)
    after = torch.cuda.memory_allocated()
    assert after == before
    assert second.data_ptr() == first.data_ptr() == again.data_ptr() and again.untyped_storage().data_ptr() == first.untyped_storage().data_ptr()
    assert info_c is info_a and info_b is not info_a
    assert torch.equal(again, kept)
    other, _, _, _ = store.target(0, 4)                            # another geometry: another buffer
    assert other.data_ptr() != first.data_ptr()


def test_store_autoscales_an_image_over_the_limit(tmp_path):
    """through ImagePoseDataset and PIL: a 1648 x 832 image is stored as the f32 (3,1600,800) autoscaled image"""
    import json

    import PIL.Image
    from taichi_3d_gaussian_splatting_amd.ImagePoseDataset import ImagePoseDataset
    u8 = pixels(1650, 840, 3, seed=15)
    PIL.Image.fromarray(u8).save(tmp_path / "big.png")
    (tmp_path / "d.json").write_text(json.dumps([dict(
        image_path=str(tmp_path / "big.png"), T_pointcloud_camera=np.eye(4).tolist(),
        camera_intrinsics=[[800.0, 0.0, 420.0], [0.0, 800.0, 825.0], [0.0, 0.0, 1.0]], camera_height=1650, camera_width=840, camera_id=0)]))
    ds = ImagePoseDataset(str(tmp_path / "d.json"))
    store = targets.TargetStore.from_dataset(ds, DEV)
    assert store.images[0].dtype == torch.float32 and tuple(store.images[0].shape) == (3, 1600, 800)
    image, _, _, info = store.target(0, 1)
    host_image, _, _, host_info = ds[0]
    assert (info.camera_height, info.camera_width) == (host_info.camera_height, host_info.camera_width) == (1600, 800)
    assert torch.equal(info.camera_intrinsics.cpu(), host_info.camera_intrinsics)
    want = resample_ref.resize_antialias(resample_ref.to_float(u8[:1648, :832]), (1600, 807), (1600, 800))
    compare(image, want, ABS_TOL)
    half, _, _, _ = store.target(0, 2)                             # the second source format: f32 CHW in, f32 CHW out
    compare(half, resample_ref.resize_antialias(want, (800, 400), (800, 400)), ABS_TOL + 2e-6)
