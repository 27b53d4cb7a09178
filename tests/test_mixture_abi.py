"""CPU: the C ABI of the scene-as-mixture calls (include/gs_mixture.h) and their binding (mixture.py)."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gs_mixture.h")
PKG = os.path.join(ROOT, "taichi_3d_gaussian_splatting_amd")
SOURCE = os.path.join(PKG, "csrc", "k_mixture.hip")
NAMES = ["gs_mixture_fourier", "gs_mixture_log_density"]


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w ]*?[\w*])\s+(gs_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        types = [re.sub(r"\bconst\b|\s", "", re.match(r"(.*?)(\w+)$", p.strip()).group(1)) for p in params.split(",")]
        protos[name] = (ret.strip(), types)
    return protos


def _define(text, name):
    return int(re.search(r"#define\s+" + name + r"\s+(\d+)", text).group(1))


def test_header_is_plain_c99_and_declares_the_two_functions(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(f'#include "{HEADER}"\n'
                   'int main(void) {\n'
                   '  int (*d)(gs_ctx*, const float*, const float*, const int8_t*, int64_t, const float*, int64_t, float*, gs_stream)\n'
                   '      = gs_mixture_log_density;\n'
                   '  int (*f)(gs_ctx*, const float*, const float*, const int8_t*, int64_t, const float*, int64_t, const float*, float*,\n'
                   '           gs_stream) = gs_mixture_fourier;\n'
                   '  (void)d; (void)f; return GS_MIXTURE_MAX_POINTS > 0 && GS_MIXTURE_MAX_QUERIES > 0 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", str(src), "-o", str(tmp_path / "probe.o")])
    assert sorted(_prototypes()) == NAMES


def test_library_exports_the_symbols_and_the_main_header_is_unchanged():
    from taichi_3d_gaussian_splatting_amd import _native
    L = _native.lib()
    for n in NAMES:
        assert hasattr(L, n), f"libgsrast.so does not export {n}"
        assert n not in _native.SYMBOLS
    assert L.gs_abi_version() == _native.ABI_VERSION == 9
    names = L.gs_kernel_names().decode().split(",")
    assert len(names) == 13 and not any("mix" in n for n in names)
    main = open(os.path.join(ROOT, "include", "gs_rasterizer.h")).read()
    assert "mixture" not in main.lower()
    assert len(_native.SYMBOLS) == 33


def test_argtypes_match_the_prototypes():
    from taichi_3d_gaussian_splatting_amd import _native, mixture
    mixture._bind()
    L = _native.lib()
    kinds = {"gs_ctx*": C.c_void_p, "float*": C.c_void_p, "int8_t*": C.c_void_p, "gs_stream": C.c_void_p, "int64_t": C.c_int64}
    protos = _prototypes()
    assert sorted(mixture.ARGTYPES) == NAMES
    for name in NAMES:
        ret, params = protos[name]
        assert ret == "int" and params[-1] == "gs_stream"          # _native.call() appends the stream
        assert name not in _native._STREAMLESS
        fn = getattr(L, name)
        assert fn.restype is C.c_int
        assert list(fn.argtypes) == [kinds[p] for p in params] == mixture.ARGTYPES[name]


def _calls(L, p):
    """the two calls with (ctx, arrays..., n_points, queries, n_q, out) spelled once: arrays = (point_cloud, features, queries, out)"""
    def density(ctx, pc, feat, n, x, n_x, out):
        return L.gs_mixture_log_density(ctx, pc, feat, None, n, x, n_x, out, None)

    def transform(ctx, pc, feat, n, k, n_k, out, centre=p):
        return L.gs_mixture_fourier(ctx, pc, feat, None, n, k, n_k, centre, out, None)
    return density, transform


def test_refuses_bad_arguments_without_a_gpu():
    """argument checks come before anything that needs a device"""
    from taichi_3d_gaussian_splatting_amd import _native, mixture
    mixture._bind()
    L = _native.lib()
    buf = (C.c_float * 256)()
    p = C.cast(buf, C.c_void_p)
    ctx = C.c_void_p(8)          # a context handle that is never dereferenced: every call below is refused, or found empty, before that
    for call in _calls(L, p):
        assert call(None, p, p, 2, p, 2, p) == -1                    # GS_ERR_INVALID_ARGUMENT
        assert b"NULL" in L.gs_last_error()
        for n in (-1, 2 ** 30 + 1, 2 ** 31):
            assert call(ctx, p, p, n, p, 2, p) == -1, n
            assert b"n_points" in L.gs_last_error()
            assert call(ctx, p, p, 2, p, n, p) == -1, n
            assert b"n_x" in L.gs_last_error() or b"n_k" in L.gs_last_error()
        for pc, feat, q, out in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None), (None, None, None, None)):
            assert call(ctx, pc, feat, 2, q, 2, out) == -1
            assert b"NULL" in L.gs_last_error()
        # nothing to do is not an error, with or without pointers
        assert call(ctx, None, None, 0, None, 0, None) == 0
        assert call(ctx, p, p, 2, None, 0, None) == 0
        assert call(ctx, None, None, 0, p, 2, p) == 0
    assert _calls(L, p)[1](ctx, p, p, 2, p, 2, p, centre=None) == -1
    assert b"NULL" in L.gs_last_error()


def test_limits_and_blocking_agree_between_the_header_the_kernels_and_python():
    from taichi_3d_gaussian_splatting_amd import mixture
    header, src = open(HEADER).read(), open(SOURCE).read()
    assert _define(header, "GS_MIXTURE_MAX_POINTS") == mixture.MAX_POINTS == 2 ** 30
    assert _define(header, "GS_MIXTURE_MAX_QUERIES") == mixture.MAX_QUERIES == 2 ** 30
    assert _define(src, "GS_MIX_POINTS_PER_WG") == mixture.POINTS_PER_WORKGROUP
    assert _define(src, "GS_MIX_POINTS_PER_WG") == 256 * _define(src, "GS_MIX_LANE_POINTS")
    assert _define(src, "GS_MIX_CHUNK") == mixture.COMPONENTS_PER_CHUNK
    math_header = open(os.path.join(PKG, "csrc", "gs_mixture_math.h")).read()
    assert _define(math_header, "GS_MIX_NFEAT") == mixture.N_FEATURES == 56


def test_cpu_tensors_are_refused_naming_the_gpu():
    from taichi_3d_gaussian_splatting_amd import mixture
    scene = (torch.zeros(10, 3), torch.zeros(10, 56), torch.zeros(10, dtype=torch.int8))
    x = torch.zeros(4, 3)
    for fn in (mixture.log_density, mixture.density):
        with pytest.raises(ValueError, match="GPU"):
            fn(scene, x)
    with pytest.raises(ValueError, match="GPU"):
        mixture.fourier(scene, x, torch.zeros(3))
    for fn in (mixture.density_volume, mixture.fourier_volume, mixture.compare_volume_to_transform, mixture.ft_grab_scene):
        with pytest.raises(ValueError, match="GPU"):
            fn(scene, 4, torch.tensor([[-1.0] * 3, [1.0] * 3]))
    with pytest.raises(ValueError, match=r"\(P,3\)"):
        mixture.log_density(scene, torch.zeros(4, 2))


def test_the_module_is_exported_and_adds_no_trainer_field():
    import taichi_3d_gaussian_splatting_amd as pkg
    assert pkg.mixture.ft_grab_scene is pkg.mixture.compare_volume_to_transform
    assert not any("mixture" in f.lower() or "ftgmm" in f.lower() for f in vars(pkg.GaussianPointCloudTrainer.TrainConfig))


def test_product_sources_do_not_mention_the_checker():
    for path in (os.path.join(PKG, "mixture.py"), SOURCE, os.path.join(PKG, "csrc", "gs_mixture_math.h"), HEADER):
        assert "oracle" not in open(path).read().lower(), path
