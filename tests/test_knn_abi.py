"""CPU: the C ABI of the exact k-nearest-neighbour query (include/gs_knn.h) and its binding (knn.py)."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gs_knn.h")
PKG = os.path.join(ROOT, "taichi_3d_gaussian_splatting_amd")
NAMES = ["gs_knn"]


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w ]*?[\w*])\s+(gs_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        types = [re.sub(r"\bconst\b|\s", "", re.match(r"(.*?)(\w+)$", p.strip()).group(1)) for p in params.split(",")]
        protos[name] = (ret.strip(), types)
    return protos


def test_header_is_plain_c99_and_declares_the_one_function(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(f'#include "{HEADER}"\n'
                   'int main(void) {\n'
                   '  int (*f)(gs_ctx*, const float*, const int8_t*, int64_t, int32_t, float*, int32_t*, gs_stream) = gs_knn;\n'
                   '  (void)f; return GS_KNN_MAX_POINTS > 0 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", str(src), "-o", str(tmp_path / "probe.o")])
    assert sorted(_prototypes()) == NAMES


def test_library_exports_the_symbol_and_the_main_header_is_unchanged():
    from taichi_3d_gaussian_splatting_amd import _native
    L = _native.lib()
    for n in NAMES:
        assert hasattr(L, n), f"libgsrast.so does not export {n}"
        assert n not in _native.SYMBOLS
    assert L.gs_abi_version() == _native.ABI_VERSION == 9
    assert len(L.gs_kernel_names().decode().split(",")) == 13
    main = open(os.path.join(ROOT, "include", "gs_rasterizer.h")).read()
    assert "knn" not in main.lower()
    assert len(_native.SYMBOLS) == 33


def test_argtypes_match_the_prototype():
    from taichi_3d_gaussian_splatting_amd import _native, knn
    knn._bind()
    L = _native.lib()
    kinds = {"gs_ctx*": C.c_void_p, "float*": C.c_void_p, "int8_t*": C.c_void_p, "int32_t*": C.c_void_p, "gs_stream": C.c_void_p,
             "int32_t": C.c_int32, "int64_t": C.c_int64}
    ret, params = _prototypes()["gs_knn"]
    assert ret == "int" and params[-1] == "gs_stream"          # _native.call() appends the stream
    assert "gs_knn" not in _native._STREAMLESS
    assert L.gs_knn.restype is C.c_int
    assert list(L.gs_knn.argtypes) == [kinds[p] for p in params] == knn.ARGTYPES["gs_knn"]


def test_refuses_bad_arguments_without_a_gpu():
    """argument checks come before anything that needs a device"""
    from taichi_3d_gaussian_splatting_amd import _native, knn
    knn._bind()
    L = _native.lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert L.gs_knn(None, p, None, 4, 3, p, p, None) == -1            # GS_ERR_INVALID_ARGUMENT
    assert b"NULL" in L.gs_last_error()
    # a context handle that is never dereferenced: all of these are refused (or found to be empty) before the context is looked at
    ctx = C.c_void_p(8)
    for k in (0, 9, -1):
        assert L.gs_knn(ctx, p, None, 4, k, p, p, None) == -1, k
        assert b"k must be in [1, 8]" in L.gs_last_error()
    for n in (-1, 2 ** 30 + 1, 2 ** 31):
        assert L.gs_knn(ctx, p, None, n, 3, p, p, None) == -1, n
        assert b"n_points" in L.gs_last_error()
    for xyz, d2 in ((None, p), (p, None), (None, None)):
        assert L.gs_knn(ctx, xyz, None, 4, 3, d2, p, None) == -1
        assert b"NULL" in L.gs_last_error()
    # nothing to do is not an error, with or without pointers
    assert L.gs_knn(ctx, None, None, 0, 3, None, None, None) == 0
    assert L.gs_knn(ctx, p, None, 0, 8, p, p, None) == 0


def test_limits_agree_between_the_header_the_kernels_and_python():
    from taichi_3d_gaussian_splatting_amd import knn
    header = open(HEADER).read()
    assert int(re.search(r"#define\s+GS_KNN_MAX_POINTS\s+(\d+)", header).group(1)) == 2 ** 30
    src = open(os.path.join(PKG, "csrc", "k_knn.hip")).read()
    assert int(re.search(r"#define\s+GS_KNN_LEAF\s+(\d+)", src).group(1)) == knn.LEAF == 64
    assert knn.MAX_K == 8


def test_cpu_tensors_are_refused_naming_the_gpu():
    from taichi_3d_gaussian_splatting_amd import knn
    x = torch.zeros(10, 3)
    for fn in (knn.nearest_neighbours, knn.mean_neighbour_distance):
        with pytest.raises(ValueError, match="GPU"):
            fn(x)
    with pytest.raises(ValueError, match="k must be"):
        knn.nearest_neighbours(x, k=9)


def test_product_sources_do_not_mention_the_checker():
    for path in (os.path.join(PKG, "knn.py"), os.path.join(PKG, "GaussianPointCloudScene.py"), os.path.join(PKG, "csrc", "k_knn.hip"), HEADER):
        assert "oracle" not in open(path).read().lower(), path
