"""CPU: the C ABI of the scene bake (include/gs_compose.h) and its binding (compose.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gs_compose.h")
PKG = os.path.join(ROOT, "taichi_3d_gaussian_splatting_amd")
NAMES = ["gs_scene_bake"]
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
                   '  int (*f)(gs_ctx*, const float*, const float*, int64_t, const float*, const float*, float, const float*, float*,\n'
                   '           float*, int64_t, gs_stream) = gs_scene_bake;\n'
                   '  (void)f; return GS_BAKE_SH_FLOATS == 1 + 9 + 25 + 49 && GS_BAKE_FEATURES == 56 ? 0 : 1; }\n')
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
    assert "bake" not in main.lower()


def test_argtypes_match_the_prototype():
    from taichi_3d_gaussian_splatting_amd import _native, compose
    compose._bind()
    L = _native.lib()
    kinds = {"gs_ctx*": C.c_void_p, "float*": C.c_void_p, "gs_stream": C.c_void_p, "int64_t": C.c_int64, "float": C.c_float}
    ret, params = _prototypes()["gs_scene_bake"]
    assert ret == "int" and params[-1] == "gs_stream"          # _native.call() appends the stream
    assert "gs_scene_bake" not in _native._STREAMLESS
    assert L.gs_scene_bake.restype is C.c_int
    assert list(L.gs_scene_bake.argtypes) == [kinds[p] for p in params] == compose.ARGTYPES["gs_scene_bake"]


def test_refuses_bad_arguments_without_a_gpu():
    """argument checks come before anything that needs a device"""
    from taichi_3d_gaussian_splatting_amd import _native, compose
    compose._bind()
    f = _native.lib().gs_scene_bake
    err = _native.lib().gs_last_error
    buf = (C.c_float * (59 * 64))()                           # host memory standing in for device rows: never dereferenced
    base = C.addressof(buf)
    xyz_in, ft_in, xyz_out, ft_out = base, base + 12 * 16, base + 236 * 16, base + 248 * 16
    q, t = (C.c_float * 4)(0, 0, 0, 1), (C.c_float * 3)(0, 0, 0)
    sh = (C.c_float * 84)(*compose.sh_rotation_matrices(np.eye(3)).astype(np.float32))
    assert f(None, xyz_in, ft_in, 4, q, t, 1.0, sh, xyz_out, ft_out, 0, None) == INVALID and b"ctx is NULL" in err()
    ctx = C.c_void_p(8)       # a context handle that is never dereferenced: everything below is refused (or empty) before it is looked at
    assert f(ctx, xyz_in, ft_in, -1, q, t, 1.0, sh, xyz_out, ft_out, 0, None) == INVALID and b"negative" in err()
    assert f(ctx, xyz_in, ft_in, 4, q, t, 1.0, sh, xyz_out, ft_out, -1, None) == INVALID and b"negative" in err()
    assert f(ctx, xyz_in, ft_in, 2 ** 31, q, t, 1.0, sh, xyz_out, ft_out, 0, None) == INVALID and b"2^31" in err()
    assert f(ctx, xyz_in, ft_in, 4, q, t, 1.0, sh, xyz_out, ft_out, 2 ** 31 - 2, None) == INVALID and b"2^31" in err()
    for args in ((None, t, sh), (q, None, sh), (q, t, None)):
        assert f(ctx, xyz_in, ft_in, 4, args[0], args[1], 1.0, args[2], xyz_out, ft_out, 0, None) == INVALID and b"NULL q_A" in err()
    for s in (0.0, -1.0, float("inf"), float("nan")):
        assert f(ctx, xyz_in, ft_in, 4, q, t, s, sh, xyz_out, ft_out, 0, None) == INVALID and b"scale" in err()
    for bad in ((0, 0, 0, 0), (float("nan"), 0, 0, 1), (float("inf"), 0, 0, 1)):
        assert f(ctx, xyz_in, ft_in, 4, (C.c_float * 4)(*bad), t, 1.0, sh, xyz_out, ft_out, 0, None) == INVALID and b"q_A" in err()
    assert f(ctx, xyz_in, ft_in, 4, q, (C.c_float * 3)(0, float("inf"), 0), 1.0, sh, xyz_out, ft_out, 0, None) == INVALID and b"t_A" in err()
    bad_sh = (C.c_float * 84)(*sh)
    bad_sh[40] = float("nan")
    assert f(ctx, xyz_in, ft_in, 4, q, t, 1.0, bad_sh, xyz_out, ft_out, 0, None) == INVALID and b"sh_matrices" in err()
    for arrays in ((None, ft_in, xyz_out, ft_out), (xyz_in, None, xyz_out, ft_out), (xyz_in, ft_in, None, ft_out), (xyz_in, ft_in, xyz_out, None)):
        assert f(ctx, arrays[0], arrays[1], 4, q, t, 1.0, sh, arrays[2], arrays[3], 0, None) == INVALID and b"NULL array" in err()
    # aliasing: in place, partly overlapping, crosswise, and only through the row offset
    assert f(ctx, xyz_in, ft_in, 4, q, t, 1.0, sh, xyz_in, ft_out, 0, None) == INVALID and b"overlap" in err()
    assert f(ctx, xyz_in, ft_in, 4, q, t, 1.0, sh, xyz_out, ft_in, 0, None) == INVALID and b"overlap" in err()
    assert f(ctx, xyz_in, ft_in, 4, q, t, 1.0, sh, xyz_out, ft_in + 224 * 3, 0, None) == INVALID and b"overlap" in err()
    assert f(ctx, xyz_in, ft_in, 4, q, t, 1.0, sh, ft_in + 8, ft_out, 0, None) == INVALID and b"overlap" in err()
    assert f(ctx, xyz_in, ft_in + 224 * 4, 4, q, t, 1.0, sh, xyz_out, ft_in, 4, None) == INVALID and b"overlap" in err()
    # nothing to do is not an error, with or without arrays
    assert f(ctx, None, None, 0, q, t, 1.0, sh, None, None, 0, None) == 0
    assert f(ctx, xyz_in, ft_in, 0, q, t, 2.5, sh, xyz_in, ft_in, 7, None) == 0


def test_limits_agree_between_the_header_the_kernel_and_python():
    from taichi_3d_gaussian_splatting_amd import compose
    assert _define("GS_BAKE_FEATURES") == compose.FEATURES == 56
    assert _define("GS_BAKE_SH_FLOATS") == compose.SH_FLOATS == sum((2 * l + 1) ** 2 for l in range(4))
    assert _define("GS_BAKE_ROWS_PER_BLOCK") == compose.ROWS_PER_BLOCK == 64
    common = open(os.path.join(PKG, "csrc", "gs_common.h")).read()
    assert "float sh[84]" in common
    # static LDS of the kernel: a padded row per lane
    assert compose.ROWS_PER_BLOCK * (compose.FEATURES + 1) * 4 <= 64 * 1024


def test_cpu_tensors_and_bad_placements_are_refused():
    from taichi_3d_gaussian_splatting_amd import compose
    with pytest.raises(ValueError, match="GPU"):
        compose.scene_bake(torch.zeros(4, 3), torch.zeros(4, 56), [0, 0, 0, 1], [0, 0, 0])
    with pytest.raises(ValueError, match="GPU"):
        compose.SceneComposition([(np.zeros((2, 3)), np.zeros((2, 56)))], device="cpu")
    for q, t, s, what in (([0, 0, 0, 0], [0, 0, 0], 1.0, "quaternion"), ([0, 0, 0, 1], [0, np.nan, 0], 1.0, "translation"),
                          ([0, 0, 0, 1], [0, 0, 0], 0.0, "scale"), ([0, 0, 0, 1], [0, 0, 0], float("inf"), "scale")):
        with pytest.raises(ValueError, match=what):
            compose._placement(q, t, s)
    q, t, s = compose._placement([0, 0, 3.0, 4.0], [1, 2, 3], 2)
    assert np.allclose(q, [0, 0, 0.6, 0.8]) and s == 2.0


def test_product_sources_do_not_mention_the_checker():
    for path in (os.path.join(PKG, "compose.py"), os.path.join(PKG, "csrc", "k_compose.hip"), HEADER):
        assert "oracle" not in open(path).read().lower(), path
