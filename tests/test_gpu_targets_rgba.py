"""GPU (-m gpu): gs_image_resample_rgba (include/gs_targets_rgba.h), raw and through targets.py: planes 0..2 bit for bit
what gs_image_resample writes, plane 3 (the weight) against the float64 restatement of the same filter on channel 3
(tests/weighted_loss_ref.weight_plane), within the resample bar of tests/test_gpu_targets.py (2e-6), bit-exact at factor 1.

Cases: factors 1, 2, 4 and 8; outputs at, one past and beyond the 16x64 workgroup tile; a crop that ends before the resize;
a row pitch that is no multiple of 16 (nor of 4) with an output no 16-byte store can write; the f32 (4,H,W) source; the
words around the destination; TargetStore's image and weight as views of one buffer; a mask file and an alpha channel that
hold the same bytes."""
import json

import numpy as np
import pytest
import torch

import weighted_loss_ref as wref
from taichi_3d_gaussian_splatting_amd import targets
from test_gpu_targets import GUARD_BITS, on_device, pixels, store_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ABS_TOL = 2e-6


def guarded_out(h, w):
    guard = 2 * max(w, 1) + 4
    guard += (-guard) % 4
    buf = torch.full((guard + 4 * h * w + guard,), GUARD_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    return buf, buf[guard:guard + 4 * h * w].view(4, h, w), guard


def run(src, size_full, size_out):
    """-> the (4,h,w) result, after checking the guards around it and planes 0..2 against gs_image_resample bit for bit"""
    buf, out, guard = guarded_out(*size_out)
    got = targets.image_resample(src, size_full, size_out, out=out, alpha=True)
    assert got.data_ptr() == out.data_ptr()
    rgb = targets.image_resample(src, size_full, size_out)
    torch.cuda.synchronize()
    words = buf.view(torch.int32)
    assert bool((words[:guard] == GUARD_BITS).all()) and bool((words[guard + out.numel():] == GUARD_BITS).all()), "the kernel wrote outside its output"
    assert torch.equal(out[:3], rgb), "planes 0..2 differ from gs_image_resample"
    return out


def compare_weight(plane, want, tol=ABS_TOL):
    got = plane.cpu().numpy().astype(np.float64)
    assert got.shape == want.shape and np.isfinite(got).all()
    err = np.abs(got - want)
    print("plane 3 max error", float(err.max()))
    for name, e in {"rows 0-1": err[:2], "rows -2,-1": err[-2:], "columns 0-1": err[:, :2], "columns -2,-1": err[:, -2:]}.items():
        assert e.max() <= tol, (name, float(e.max()))
    assert err.max() <= tol, float(err.max())


def alpha_exact(u8):
    """channel 3 / 255 as the kernel forms it: true division in f32 (taken on the CPU)"""
    return torch.from_numpy(np.array(u8[..., 3])).float().div(255).to(DEV)


@pytest.mark.parametrize("factor", [1, 2, 4, 8])
def test_factors(factor):
    u8 = pixels(128, 192, 4, seed=20)
    h_full, w_full, h, w = targets.downsampled_geometry(128, 192, factor)
    assert (h, w) == {1: (128, 192), 2: (64, 96), 4: (32, 48), 8: (16, 16)}[factor]
    out = run(on_device(u8), (h_full, w_full), (h, w))
    compare_weight(out[3], wref.weight_plane(u8, (h_full, w_full), (h, w)))
    if factor == 1:
        assert torch.equal(out[3], alpha_exact(u8))


@pytest.mark.parametrize("h,w", [(16, 64), (17, 65), (48, 80)], ids=["16x64", "17x65", "48x80"])
def test_outputs_at_the_tile_edges(h, w):
    u8 = pixels(2 * h + 1, 3 * w + 2, 4, seed=21)
    out = run(on_device(u8, pitch=((3 * w + 2) * 4 + 15) // 16 * 16), (h, w), (h, w))
    compare_weight(out[3], wref.weight_plane(u8, (h, w)))
    cropped = run(on_device(u8), (h, w), (h - 1, w - 3))           # the crop ends before the resize does: the same bits
    assert torch.equal(cropped, out[:, :h - 1, :w - 3])


def test_row_pitch_that_is_no_multiple_of_16():
    u8 = pixels(37, 53, 4, seed=22)
    src = on_device(u8, pitch=215)
    assert src.stride(0) == 215 and 215 % 16 != 0 and 215 % 4 != 0
    out = run(src, (9, 13), (9, 13))                               # w_out = 13: no 16-byte store
    compare_weight(out[3], wref.weight_plane(u8, (9, 13)))
    shifted = torch.zeros(37 * 215 + 3, dtype=torch.uint8, device=DEV)[3:].as_strided((37, 53, 4), (215, 4, 1))
    assert shifted.data_ptr() % 4 == 3
    shifted.copy_(src)
    assert torch.equal(run(shifted, (9, 13), (9, 13)), out)
    same = run(on_device(u8, pitch=53 * 4 + 12), (37, 53), (32, 48))          # factor 1 from a pitch of 224
    assert torch.equal(same[3], alpha_exact(u8)[:32, :48])


@pytest.mark.parametrize("size_full,size_out", [((32, 48), (32, 48)), ((21, 30), (16, 16)), ((64, 96), (48, 80))])
def test_f32_four_plane_source(size_full, size_out):
    image = np.random.default_rng(4).uniform(0.0, 1.0, (4, 64, 96)).astype(np.float32)
    src = torch.from_numpy(image).to(DEV)
    out = run(src, size_full, size_out)
    if size_full == (64, 96):
        assert torch.equal(out, src[:, :size_out[0], :size_out[1]])  # equal sizes: the input, cropped, bit for bit
    import resample_ref
    compare_weight(out[3], resample_ref.resize_antialias(image[3:4], size_full, size_out)[0])


def test_three_channel_sources_and_wrong_outputs_are_refused():
    rgb = on_device(pixels(64, 96, 3))
    with pytest.raises(ValueError, match="four-channel"):
        targets.image_resample(rgb, (32, 48), alpha=True)
    rgba = on_device(pixels(64, 96, 4))
    with pytest.raises(ValueError, match=r"\(4,32,48\)"):
        targets.image_resample(rgba, (32, 48), out=torch.empty(3, 32, 48, device=DEV), alpha=True)
    assert tuple(targets.image_resample(rgba, (32, 48), (0, 48), alpha=True).shape) == (4, 0, 48)
    torch.cuda.synchronize()


def test_target_store_hands_out_views_of_one_buffer():
    images = [pixels(80, 112, 4, seed=23), pixels(80, 112, 4, seed=24)]
    store, _ = store_of(images)
    for f in (1, 2):
        plain = store.target(0, f)[0].clone()
        image, q, t, info, weight = store.target(0, f, with_weight=True)
        assert torch.equal(image, plain)
        assert image.is_contiguous() and weight.is_contiguous() and tuple(weight.shape) == tuple(image.shape[1:])
        assert image.untyped_storage().data_ptr() == weight.untyped_storage().data_ptr()
        assert weight.data_ptr() == image.data_ptr() + 4 * image.numel()
        assert (info.camera_height, info.camera_width) == tuple(weight.shape)
        compare_weight(weight, wref.weight_plane(images[0][:80, :112], (80 // f, 112 // f), tuple(weight.shape)))
    assert torch.equal(store.target(0, 1, with_weight=True)[4], alpha_exact(images[0]))
    torch.cuda.synchronize()
    first = store.target(0, 2, with_weight=True)
    kept = first[4].clone()
    before = torch.cuda.memory_allocated()
    second = store.target(1, 2, with_weight=True)
    again = store.target(0, 2, with_weight=True)
    assert torch.cuda.memory_allocated() == before                # no allocation after the first use of a geometry
    assert second[0].data_ptr() == first[0].data_ptr() == again[0].data_ptr() and torch.equal(again[4], kept)
    assert store.target(0, 2)[0].data_ptr() != first[0].data_ptr()          # the three-plane buffer is its own
    rgb_store, _ = store_of([pixels(80, 112, 3, seed=25)])
    with pytest.raises(ValueError, match="four-channel"):
        rgb_store.target(0, 1, with_weight=True)


def _dataset(tmp_path, name, image, mask=None):
    import PIL.Image
    from taichi_3d_gaussian_splatting_amd.ImagePoseDataset import ImagePoseDataset
    PIL.Image.fromarray(image).save(tmp_path / f"{name}.png")
    record = dict(image_path=str(tmp_path / f"{name}.png"), T_pointcloud_camera=np.eye(4).tolist(),
                  camera_intrinsics=[[100.0, 0.0, 56.0], [0.0, 100.0, 40.0], [0.0, 0.0, 1.0]], camera_height=image.shape[0],
                  camera_width=image.shape[1], camera_id=0)
    if mask is not None:
        PIL.Image.fromarray(mask, mode="L").save(tmp_path / f"{name}_mask.png")
        record["mask_path"] = str(tmp_path / f"{name}_mask.png")
    (tmp_path / f"{name}.json").write_text(json.dumps([record]))
    return ImagePoseDataset(str(tmp_path / f"{name}.json"))


def test_a_mask_file_and_an_alpha_channel_give_the_same_weight(tmp_path):
    rgba = np.array(pixels(83, 115, 4, seed=26))
    from_alpha = targets.TargetStore.from_dataset(_dataset(tmp_path, "rgba", rgba), DEV, mask_source="alpha")
    from_file = targets.TargetStore.from_dataset(_dataset(tmp_path, "rgb", rgba[..., :3].copy(), rgba[..., 3].copy()), DEV, mask_source="file")
    for f in (1, 2):
        a, b = from_alpha.target(0, f, with_weight=True), from_file.target(0, f, with_weight=True)
        assert tuple(a[4].shape) == (80 // f // 16 * 16, 112 // f // 16 * 16)
        assert torch.equal(a[0], b[0]) and torch.equal(a[4], b[4])
    assert torch.equal(from_file.target(0, 1, with_weight=True)[4], alpha_exact(rgba)[:80, :112])
    # mask_erode shrinks the mask once, at load
    binary = np.zeros((83, 115), np.uint8)
    binary[20:60, 30:90] = 255
    eroded = targets.TargetStore.from_dataset(_dataset(tmp_path, "hole", rgba[..., :3].copy(), binary), DEV, mask_source="file", mask_erode=5)
    want = torch.zeros(80, 112, device=DEV)
    want[25:55, 35:85] = 1.0
    assert torch.equal(eroded.target(0, 1, with_weight=True)[4], want)
    with pytest.raises(ValueError, match="mask_path"):
        targets.TargetStore.from_dataset(_dataset(tmp_path, "nomask", rgba[..., :3].copy()), DEV, mask_source="file")
    with pytest.raises(ValueError, match="alpha"):
        targets.TargetStore.from_dataset(_dataset(tmp_path, "noalpha", rgba[..., :3].copy()), DEV, mask_source="alpha")


def test_store_autoscales_an_rgba_image_over_the_limit_with_its_alpha(tmp_path):
    """a 1648 x 832 RGBA image is stored as the f32 (4,1600,800) autoscaled image: planes 0..2 as without a mask, plane 3 the
    alpha through the same resize; targets at factor 2 then come from the f32 four-plane source"""
    import resample_ref
    u8 = np.array(pixels(1650, 840, 4, seed=27))
    store = targets.TargetStore.from_dataset(_dataset(tmp_path, "big", u8), DEV, mask_source="alpha")
    plain = targets.TargetStore.from_dataset(_dataset(tmp_path, "big", u8), DEV)
    assert store.images[0].dtype == torch.float32 and tuple(store.images[0].shape) == (4, 1600, 800)
    assert torch.equal(store.images[0][:3], plain.images[0])
    image, _, _, info, weight = store.target(0, 1, with_weight=True)
    assert (info.camera_height, info.camera_width) == (1600, 800) and torch.equal(image, plain.target(0, 1)[0])
    want = wref.weight_plane(u8[:1648, :832], (1600, 807), (1600, 800))
    compare_weight(weight, want)
    half = store.target(0, 2, with_weight=True)
    assert torch.equal(half[0], plain.target(0, 2)[0])
    compare_weight(half[4], resample_ref.resize_antialias(want[None], (800, 400), (800, 400))[0], ABS_TOL + 2e-6)
