"""CPU: the C ABI of the 8-bit frame conversion (include/gs_frames.h) and its binding (frames.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gs_frames.h")
PKG = os.path.join(ROOT, "taichi_3d_gaussian_splatting_amd")
NAMES = ["gs_frame_to_u8"]
INVALID = -1                                                      # GS_ERR_INVALID_ARGUMENT


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w ]*?[\w*])\s+(gs_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        types = [re.sub(r"\bconst\b|\s", "", re.match(r"(.*?)(\w+)$", p.strip()).group(1)) for p in params.split(",")]
        protos[name] = (ret.strip(), types)
    return protos


def _define(name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, open(HEADER).read()).group(1))


def test_header_is_plain_c99_and_declares_the_one_function(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(f'#include "{HEADER}"\n'
                   'int main(void) {\n'
                   '  int (*f)(gs_ctx*, const float*, int32_t, int32_t, int32_t, uint8_t*, int64_t, const uint8_t*, int32_t, int64_t,\n'
                   '           int64_t*, gs_stream) = gs_frame_to_u8;\n'
                   '  (void)f; return GS_FRAME_RGB_TRUNC == 0 && GS_FRAME_RGB_ROUND == 1 && GS_FRAME_DEPTH_CMAP == 2 ? 0 : 1; }\n')
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
    assert "frame_to_u8" not in main.lower()


def test_argtypes_match_the_prototype():
    from taichi_3d_gaussian_splatting_amd import _native, frames
    frames._bind()
    L = _native.lib()
    kinds = {"gs_ctx*": C.c_void_p, "float*": C.c_void_p, "uint8_t*": C.c_void_p, "int64_t*": C.c_void_p, "gs_stream": C.c_void_p,
             "int32_t": C.c_int32, "int64_t": C.c_int64}
    ret, params = _prototypes()["gs_frame_to_u8"]
    assert ret == "int" and params[-1] == "gs_stream"          # _native.call() appends the stream
    assert "gs_frame_to_u8" not in _native._STREAMLESS
    assert L.gs_frame_to_u8.restype is C.c_int
    assert list(L.gs_frame_to_u8.argtypes) == [kinds[p] for p in params] == frames.ARGTYPES["gs_frame_to_u8"]


def test_refuses_bad_arguments_without_a_gpu():
    """argument checks come before anything that needs a device"""
    from taichi_3d_gaussian_splatting_amd import _native, frames
    frames._bind()
    f = _native.lib().gs_frame_to_u8
    err = _native.lib().gs_last_error
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    T = frames.RGB_TRUNC
    assert f(None, p, T, 16, 16, p, 48, None, 0, 0, None, None) == INVALID and b"ctx is NULL" in err()
    ctx = C.c_void_p(8)       # a context handle that is never dereferenced: everything below is refused (or empty) before it is looked at
    for mode in (-1, 3, 7):
        assert f(ctx, p, mode, 16, 16, p, 48, None, 0, 0, None, None) == INVALID and b"unknown mode" in err()
    for h, w in ((-1, 16), (16, -1), (2 ** 15 + 1, 16), (16, 2 ** 15 + 1)):
        assert f(ctx, p, T, h, w, p, 2 ** 20, None, 0, 0, None, None) == INVALID and b"size" in err()
    assert f(ctx, p, T, 16, 16, p, 47, None, 0, 0, None, None) == INVALID and b"dst_row_pitch_bytes" in err()
    assert f(ctx, p, frames.DEPTH_CMAP, 16, 17, p, 50, None, 0, 0, None, None) == INVALID and b"dst_row_pitch_bytes" in err()
    for ch in (0, 1, 2, 5):
        assert f(ctx, p, T, 16, 16, p, 48, p, ch, 64, p, None) == INVALID and b"gt_channels" in err()
    assert f(ctx, p, T, 16, 16, p, 48, p, 3, 47, p, None) == INVALID and b"gt_row_pitch_bytes" in err()
    assert f(ctx, p, T, 16, 16, p, 48, p, 4, 63, p, None) == INVALID and b"gt_row_pitch_bytes" in err()
    assert f(ctx, p, T, 16, 16, p, 48, p, 3, 48, None, None) == INVALID and b"needs the sse word" in err()
    assert f(ctx, p, T, 16, 16, p, 48, None, 0, 0, p, None) == INVALID and b"needs a ground truth" in err()
    for src, dst in ((None, p), (p, None)):
        assert f(ctx, src, T, 16, 16, dst, 48, None, 0, 0, None, None) == INVALID and b"NULL src or dst" in err()
    # nothing to do is not an error, with or without pointers
    assert f(ctx, None, T, 0, 16, None, 48, None, 0, 0, None, None) == 0
    assert f(ctx, p, frames.RGB_ROUND, 16, 0, p, 0, None, 0, 0, None, None) == 0
    assert f(ctx, None, frames.DEPTH_CMAP, 0, 0, None, 0, None, 0, 0, None, None) == 0


def test_limits_agree_between_the_header_the_kernel_and_python():
    from taichi_3d_gaussian_splatting_amd import frames
    assert (_define("GS_FRAME_RGB_TRUNC"), _define("GS_FRAME_RGB_ROUND"), _define("GS_FRAME_DEPTH_CMAP")) == \
        (frames.RGB_TRUNC, frames.RGB_ROUND, frames.DEPTH_CMAP)
    assert _define("GS_FRAME_MAX_SIZE") == frames.MAX_SIZE == 2 ** 15
    assert _define("GS_FRAME_BYTES_PER_THREAD") == frames.BYTES_PER_THREAD == 16
    # a workgroup's sum of squared differences fits 32 bits, a frame's 63: the sum is exact
    assert 256 * frames.BYTES_PER_THREAD * 255 ** 2 < 2 ** 32
    assert frames.MAX_SIZE ** 2 * 3 * 255 ** 2 < 2 ** 63
    assert 1 <= frames.MAX_WRITER_THREADS <= 16


def test_cpu_tensors_and_bad_layouts_are_refused():
    from taichi_3d_gaussian_splatting_amd import frames
    with pytest.raises(ValueError, match="GPU"):
        frames.frame_to_u8(torch.zeros(16, 16, 3))
    with pytest.raises(ValueError, match="GPU"):
        frames.FrameSink(None, device="cpu")
    with pytest.raises(ValueError, match="format"):
        frames.FrameSink(None, fmt="jpg")


def test_psnr_from_sse():
    from taichi_3d_gaussian_splatting_amd import frames
    got = frames.psnr_from_sse([0, 48 * 64 * 3 * 255 ** 2, 48 * 64 * 3], 48 * 64 * 3)
    assert np.isinf(got[0]) and got[1] == 0.0 and abs(got[2] - 20 * np.log10(255.0)) < 1e-12


def test_product_sources_do_not_mention_the_checker():
    for path in (os.path.join(PKG, "frames.py"), os.path.join(PKG, "csrc", "k_frames.hip"), HEADER):
        assert "oracle" not in open(path).read().lower(), path
