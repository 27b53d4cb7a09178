"""CPU: the C ABI of the four-plane target resampler (include/gs_targets_rgba.h), its binding (targets.py), the dataset's
mask column and the mask helpers of the store."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gs_targets_rgba.h")
NAMES = ["gs_image_resample_rgba"]
INVALID = -1                                                      # GS_ERR_INVALID_ARGUMENT


def _prototypes(header=HEADER):
    src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w ]*?[\w*])\s+(gs_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        types = [re.sub(r"\bconst\b|\s", "", re.match(r"(.*?)(\w+)$", p.strip()).group(1)) for p in params.split(",")]
        protos[name] = (ret.strip(), types)
    return protos


def test_header_is_plain_c99_and_declares_the_one_function(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(f'#include "{HEADER}"\n'
                   'int main(void) {\n'
                   '  int (*f)(gs_ctx*, const void*, int32_t, int32_t, int32_t, int32_t, int64_t, int32_t, int32_t, int32_t, int32_t,\n'
                   '           float*, gs_stream) = gs_image_resample_rgba;\n'
                   '  (void)f; return GS_IMAGE_U8_HWC == 0 && GS_IMAGE_F32_CHW == 1 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", str(src), "-o", str(tmp_path / "probe.o")])
    assert sorted(_prototypes()) == NAMES


def test_library_exports_the_symbol_and_the_other_headers_are_unchanged():
    from taichi_3d_gaussian_splatting_amd import _native
    L = _native.lib()
    for n in NAMES:
        assert hasattr(L, n), f"libgsrast.so does not export {n}"
        assert n not in _native.SYMBOLS
    assert L.gs_abi_version() == _native.ABI_VERSION == 9
    main = open(os.path.join(ROOT, "include", "gs_rasterizer.h")).read()
    assert "resample" not in main.lower() and "rgba" not in main.lower()
    assert sorted(_prototypes(os.path.join(ROOT, "include", "gs_targets.h"))) == ["gs_image_resample"]


def test_argtypes_match_the_prototype_and_gs_image_resamples():
    from taichi_3d_gaussian_splatting_amd import _native, targets
    targets._bind()
    L = _native.lib()
    kinds = {"gs_ctx*": C.c_void_p, "void*": C.c_void_p, "float*": C.c_void_p, "gs_stream": C.c_void_p,
             "int32_t": C.c_int32, "int64_t": C.c_int64}
    ret, params = _prototypes()["gs_image_resample_rgba"]
    assert ret == "int" and params[-1] == "gs_stream"          # _native.call() appends the stream
    assert "gs_image_resample_rgba" not in _native._STREAMLESS
    assert L.gs_image_resample_rgba.restype is C.c_int
    assert list(L.gs_image_resample_rgba.argtypes) == [kinds[p] for p in params] == targets.ARGTYPES["gs_image_resample_rgba"]
    assert targets.ARGTYPES["gs_image_resample_rgba"] == targets.ARGTYPES["gs_image_resample"]


def test_refuses_bad_arguments_without_a_gpu():
    """argument checks come before anything that needs a device; they are gs_image_resample's, with src_channels fixed to 4"""
    from taichi_3d_gaussian_splatting_amd import _native, targets
    targets._bind()
    f = _native.lib().gs_image_resample_rgba
    err = _native.lib().gs_last_error
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    U8, F32 = targets.FORMAT_U8_HWC, targets.FORMAT_F32_CHW
    assert f(None, p, U8, 4, 64, 96, 384, 32, 48, 32, 48, p, None) == INVALID
    assert b"gs_image_resample_rgba: ctx is NULL" in err()
    ctx = C.c_void_p(8)       # a context handle that is never dereferenced: everything below is refused (or empty) before it is looked at
    assert f(ctx, p, 2, 4, 64, 96, 384, 32, 48, 32, 48, p, None) == INVALID and b"src_format" in err()
    for ch in (0, 1, 2, 3, 5):
        assert f(ctx, p, U8, ch, 64, 96, 96 * 4, 32, 48, 32, 48, p, None) == INVALID and b"src_channels must be 4" in err(), ch
        assert f(ctx, p, F32, ch, 64, 96, 96 * 4, 32, 48, 32, 48, p, None) == INVALID and b"src_channels must be 4" in err(), ch
    for sizes in ((-1, 96, 32, 48, 32, 48), (64, 96, 32, 48, -1, 48), (64, 2 ** 15 + 1, 32, 48, 32, 48)):
        assert f(ctx, p, U8, 4, sizes[0], sizes[1], 2 ** 20, *sizes[2:], p, None) == INVALID and b"size" in err()
    assert f(ctx, p, U8, 4, 64, 96, 384, 32, 48, 33, 48, p, None) == INVALID and b"crop" in err()
    assert f(ctx, p, U8, 4, 64, 96, 383, 32, 48, 32, 48, p, None) == INVALID and b"pitch" in err()
    assert f(ctx, p, F32, 4, 64, 96, 388, 32, 48, 32, 48, p, None) == INVALID and b"pitch" in err()
    for src, dst in ((None, p), (p, None)):
        assert f(ctx, src, U8, 4, 64, 96, 384, 32, 48, 32, 48, dst, None) == INVALID and b"NULL src or dst" in err()
    for H, W, h, w in ((31, 96, 32, 48), (136, 96, 16, 48), (64, 385, 32, 48)):
        assert f(ctx, p, U8, 4, H, W, W * 4, h, w, 16, 16, p, None) == INVALID and b"scale" in err(), (H, W, h, w)
    assert f(ctx, None, U8, 4, 64, 96, 384, 32, 48, 0, 48, None, None) == 0          # nothing to do is not an error


def test_python_refuses_before_the_library_is_asked():
    from taichi_3d_gaussian_splatting_amd import targets
    with pytest.raises(ValueError, match="GPU"):
        targets.image_resample(torch.zeros(32, 48, 4, dtype=torch.uint8), (16, 24), alpha=True)
    with pytest.raises(ValueError, match="mask_source"):
        targets.TargetStore.from_dataset([], "cuda", mask_source="sky")
    with pytest.raises(ValueError, match="mask_erode"):
        targets.TargetStore.from_dataset([], "cuda", mask_erode=3)


def test_erode_mask_shrinks_by_k_pixels():
    from taichi_3d_gaussian_splatting_amd import targets
    mask = torch.zeros(40, 50, dtype=torch.uint8)
    mask[14:34, 5:30] = 255
    mask[:12, 38:] = 255                                   # in the image's corner: what lies outside does not shrink it
    assert targets.erode_mask(mask, 0) is mask
    want = torch.zeros_like(mask)
    want[19:29, 10:25] = 255
    want[:7, 43:] = 255
    out = targets.erode_mask(mask, 5)
    assert out.dtype == torch.uint8 and torch.equal(out, want)
    grey = torch.full((12, 12), 200, dtype=torch.uint8)
    grey[6, 6] = 40
    assert torch.equal(targets.erode_mask(grey, 1)[5:8, 5:8], torch.full((3, 3), 40, dtype=torch.uint8))       # a minimum filter


def test_with_mask_replaces_channel_3():
    from taichi_3d_gaussian_splatting_amd import targets
    rgb = torch.randint(0, 256, (6, 7, 3), dtype=torch.uint8)
    rgba = torch.randint(0, 256, (6, 7, 4), dtype=torch.uint8)
    mask = torch.randint(0, 256, (6, 7), dtype=torch.uint8)
    for image in (rgb, rgba):
        out = targets._with_mask(image, mask)
        assert out.shape == (6, 7, 4) and out.is_contiguous() and torch.equal(out[..., :3], image[..., :3]) and torch.equal(out[..., 3], mask)
    with pytest.raises(ValueError, match="picture's size"):
        targets._with_mask(rgb, mask[:5])
    with pytest.raises(ValueError, match="uint8"):
        targets._with_mask(rgb, mask.float())


def test_dataset_load_mask(tmp_path):
    import PIL.Image
    from taichi_3d_gaussian_splatting_amd.ImagePoseDataset import ImagePoseDataset
    rng = np.random.default_rng(0)
    image = rng.integers(0, 256, (32, 48, 3)).astype(np.uint8)
    mask = (rng.random((32, 48)) < 0.5).astype(np.uint8) * 255
    PIL.Image.fromarray(image).save(tmp_path / "a.png")
    PIL.Image.fromarray(mask, mode="L").save(tmp_path / "a_mask.png")
    record = dict(image_path=str(tmp_path / "a.png"), T_pointcloud_camera=np.eye(4).tolist(),
                  camera_intrinsics=[[50.0, 0, 24], [0, 50.0, 16], [0, 0, 1]], camera_height=32, camera_width=48, camera_id=0)
    with open(tmp_path / "plain.json", "w") as fh:
        json.dump([record], fh)
    with open(tmp_path / "masked.json", "w") as fh:
        json.dump([dict(record, mask_path=str(tmp_path / "a_mask.png")), dict(record, mask_path="")], fh)
    assert ImagePoseDataset(str(tmp_path / "plain.json")).load_mask(0) is None
    ds = ImagePoseDataset(str(tmp_path / "masked.json"))
    got = ds.load_mask(0)
    assert got.dtype == np.uint8 and got.shape == (32, 48) and np.array_equal(got, mask)
    assert ds.load_mask(1) is None
    raw = ds.load_raw(0)[0]
    assert raw.shape == (32, 48, 3) and np.array_equal(raw.numpy(), image)          # load_raw is unchanged
