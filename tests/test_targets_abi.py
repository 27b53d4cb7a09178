"""CPU: the C ABI of the target resampler (include/gs_targets.h) and its binding (targets.py)."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gs_targets.h")
PKG = os.path.join(ROOT, "taichi_3d_gaussian_splatting_amd")
NAMES = ["gs_image_resample"]
INVALID = -1                                                      # GS_ERR_INVALID_ARGUMENT


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w ]*?[\w*])\s+(gs_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        types = [re.sub(r"\bconst\b|\s", "", re.match(r"(.*?)(\w+)$", p.strip()).group(1)) for p in params.split(",")]
        protos[name] = (ret.strip(), types)
    return protos


def _define(name, text=None):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text or open(HEADER).read()).group(1))


def test_header_is_plain_c99_and_declares_the_one_function(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(f'#include "{HEADER}"\n'
                   'int main(void) {\n'
                   '  int (*f)(gs_ctx*, const void*, int32_t, int32_t, int32_t, int32_t, int64_t, int32_t, int32_t, int32_t, int32_t,\n'
                   '           float*, gs_stream) = gs_image_resample;\n'
                   '  (void)f; return GS_IMAGE_U8_HWC == 0 && GS_IMAGE_F32_CHW == 1 && GS_RESAMPLE_TILE_W > 0 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", str(src), "-o", str(tmp_path / "probe.o")])
    assert sorted(_prototypes()) == NAMES


def test_library_exports_the_symbol_and_the_main_header_is_unchanged():
    from taichi_3d_gaussian_splatting_amd import _native
    L = _native.lib()
    for n in NAMES:
        assert hasattr(L, n), f"libgsrast.so does not export {n}"
        assert n not in _native.SYMBOLS
    assert L.gs_abi_version() == _native.ABI_VERSION == 9
    main = open(os.path.join(ROOT, "include", "gs_rasterizer.h")).read()
    assert "resample" not in main.lower()


def test_argtypes_match_the_prototype():
    from taichi_3d_gaussian_splatting_amd import _native, targets
    targets._bind()
    L = _native.lib()
    kinds = {"gs_ctx*": C.c_void_p, "void*": C.c_void_p, "float*": C.c_void_p, "gs_stream": C.c_void_p,
             "int32_t": C.c_int32, "int64_t": C.c_int64}
    ret, params = _prototypes()["gs_image_resample"]
    assert ret == "int" and params[-1] == "gs_stream"          # _native.call() appends the stream
    assert "gs_image_resample" not in _native._STREAMLESS
    assert L.gs_image_resample.restype is C.c_int
    assert list(L.gs_image_resample.argtypes) == [kinds[p] for p in params] == targets.ARGTYPES["gs_image_resample"]


def test_refuses_bad_arguments_without_a_gpu():
    """argument checks come before anything that needs a device"""
    from taichi_3d_gaussian_splatting_amd import _native, targets
    targets._bind()
    f = _native.lib().gs_image_resample
    err = _native.lib().gs_last_error
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    U8, F32 = targets.FORMAT_U8_HWC, targets.FORMAT_F32_CHW
    assert f(None, p, U8, 3, 64, 96, 288, 32, 48, 32, 48, p, None) == INVALID
    assert b"ctx is NULL" in err()
    ctx = C.c_void_p(8)       # a context handle that is never dereferenced: everything below is refused (or empty) before it is looked at
    assert f(ctx, p, 2, 3, 64, 96, 288, 32, 48, 32, 48, p, None) == INVALID and b"src_format" in err()
    for ch in (0, 1, 2, 5):
        assert f(ctx, p, U8, ch, 64, 96, 96 * 4, 32, 48, 32, 48, p, None) == INVALID and b"src_channels" in err()
    for sizes in ((-1, 96, 32, 48, 32, 48), (64, 96, 32, 48, -1, 48), (64, 2 ** 15 + 1, 32, 48, 32, 48)):
        assert f(ctx, p, U8, 3, sizes[0], sizes[1], 2 ** 20, *sizes[2:], p, None) == INVALID and b"size" in err()
    assert f(ctx, p, U8, 3, 64, 96, 288, 32, 48, 33, 48, p, None) == INVALID and b"crop" in err()
    assert f(ctx, p, U8, 3, 64, 96, 288, 32, 48, 32, 49, p, None) == INVALID and b"crop" in err()
    assert f(ctx, p, U8, 3, 64, 96, 287, 32, 48, 32, 48, p, None) == INVALID and b"pitch" in err()
    assert f(ctx, p, U8, 4, 64, 96, 383, 32, 48, 32, 48, p, None) == INVALID and b"pitch" in err()
    assert f(ctx, p, F32, 3, 64, 96, 388, 32, 48, 32, 48, p, None) == INVALID and b"pitch" in err()
    for src, dst in ((None, p), (p, None)):
        assert f(ctx, src, U8, 3, 64, 96, 288, 32, 48, 32, 48, dst, None) == INVALID and b"NULL src or dst" in err()
    # the scale: no upscaling, at most 8 (136 -> 16 is 8.5; 129 -> 16 is just over), on either axis
    for H, W, h, w in ((31, 96, 32, 48), (64, 47, 32, 48), (136, 96, 16, 48), (129, 96, 16, 48), (64, 385, 32, 48)):
        assert f(ctx, p, U8, 3, H, W, W * 3, h, w, 16, 16, p, None) == INVALID, (H, W, h, w)
        assert b"scale" in err()
    # nothing to do is not an error, with or without pointers, whatever the scale
    assert f(ctx, None, U8, 3, 64, 96, 288, 32, 48, 0, 48, None, None) == 0
    assert f(ctx, p, U8, 3, 64, 96, 288, 32, 48, 32, 0, p, None) == 0
    assert f(ctx, None, F32, 3, 0, 0, 0, 0, 0, 0, 0, None, None) == 0


def test_limits_agree_between_the_header_the_kernel_and_python():
    from taichi_3d_gaussian_splatting_amd import targets
    assert _define("GS_RESAMPLE_TILE_H") == targets.TILE_H == 16
    assert _define("GS_RESAMPLE_TILE_W") == targets.TILE_W == 64
    assert _define("GS_RESAMPLE_MAX_SCALE") == targets.MAX_SCALE == 8
    assert _define("GS_RESAMPLE_MAX_SIZE") == targets.MAX_SIZE == 2 ** 15
    assert (_define("GS_IMAGE_U8_HWC"), _define("GS_IMAGE_F32_CHW")) == (targets.FORMAT_U8_HWC, targets.FORMAT_F32_CHW)
    common = open(os.path.join(PKG, "csrc", "gs_common.h")).read()
    taps, span = _define("GS_RS_MAX_TAPS", common), _define("GS_RS_MAX_SPAN", common)
    # a window holds at most 2 * scale + 1 inputs; the windows of one tile row start at most (TILE_W - 1) * scale + 1 apart
    assert taps >= 2 * targets.MAX_SCALE + 1
    assert span >= (targets.TILE_W - 1) * targets.MAX_SCALE + 1 + taps
    # static LDS of the uint8 kernel, from its own constants: staged bytes + f32 rows + the tile's tables, within 64 KB
    raw_pitch = (span * 4 + 30) // 16 * 16
    lds = 16 * raw_pitch + 16 * 3 * targets.TILE_W * 4 + (targets.TILE_W + targets.TILE_H) * (taps * 4 + 8)
    assert lds <= 64 * 1024


def test_cpu_tensors_and_bad_layouts_are_refused():
    from taichi_3d_gaussian_splatting_amd import targets
    with pytest.raises(ValueError, match="GPU"):
        targets.image_resample(torch.zeros(32, 48, 3, dtype=torch.uint8), (16, 24))
    with pytest.raises(ValueError, match="uint8 .* or a float32"):
        targets.image_resample(torch.zeros(32, 48), (16, 24))
    with pytest.raises(ValueError, match="GPU"):
        targets.TargetStore([], torch.zeros(0, 4), torch.zeros(0, 3), [], "cpu")


def test_geometry_helpers():
    from taichi_3d_gaussian_splatting_amd import targets
    assert targets.downsampled_geometry(1080, 1920, 4) == (270, 480, 256, 480)
    assert targets.downsampled_geometry(80, 112, 2) == (40, 56, 32, 48)
    # torchvision's resize(size=1024, max_size=1600): the short side to 1024 unless the long side would pass 1600
    assert targets.autoscale_size(2160, 3840) == (900, 1600)
    assert targets.autoscale_size(3000, 4000) == (1024, 1365)
    assert targets.autoscale_size(4000, 3000) == (1365, 1024)
    k = torch.tensor([[100.0, 0.5, 50.0], [0.0, 120.0, 40.0], [0.0, 0.0, 1.0]])
    assert torch.equal(targets.downsampled_intrinsics(k, 4), torch.tensor([[25.0, 0.5, 12.5], [0.0, 30.0, 10.0], [0.0, 0.0, 1.0]]))
    assert k[0, 0] == 100.0


def test_product_sources_do_not_mention_the_checker():
    for path in (os.path.join(PKG, "targets.py"), os.path.join(PKG, "csrc", "k_targets.hip"), HEADER):
        assert "oracle" not in open(path).read().lower(), path
