"""CPU: the C ABI of the feature-channel entry points (include/gs_channels.h) and their binding (channels.py)."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gs_channels.h")
PKG = os.path.join(ROOT, "taichi_3d_gaussian_splatting_amd")
NAMES = ["gs_channels_backward", "gs_channels_forward"]


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w ]*?[\w*])\s+(gs_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        types = [re.sub(r"\bconst\b|\s", "", re.match(r"(.*?)(\w+)$", p.strip()).group(1)) for p in params.split(",")]
        protos[name] = (ret.strip(), types)
    return protos


def test_header_is_plain_c99_and_declares_the_two_functions(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(f'#include <stdio.h>\n#include "{HEADER}"\n'
                   'int main(void) { int (*f)(gs_ctx*, const gs_frame*, const float*, int32_t, const int32_t*, float*, gs_stream) = 0;\n'
                   '  (void)f; printf("%d\\n", (int)GS_CHANNELS_MAX); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    from taichi_3d_gaussian_splatting_amd import channels
    assert int(subprocess.check_output([str(exe)]).decode()) == channels.GS_CHANNELS_MAX == 64
    assert sorted(_prototypes()) == NAMES


def test_library_exports_both_symbols_and_the_main_header_is_unchanged():
    from taichi_3d_gaussian_splatting_amd import _native
    L = _native.lib()
    for n in NAMES:
        assert hasattr(L, n), f"libgsrast.so does not export {n}"
        assert n not in _native.SYMBOLS
    assert L.gs_abi_version() == _native.ABI_VERSION == 9
    assert len(L.gs_kernel_names().decode().split(",")) == 13
    main = open(os.path.join(ROOT, "include", "gs_rasterizer.h")).read()
    assert "gs_channels" not in main and "GS_CHANNELS" not in main


def test_argtypes_match_the_prototypes():
    from taichi_3d_gaussian_splatting_amd import _native, channels
    channels._bind()
    L = _native.lib()
    kinds = {"gs_ctx*": C.c_void_p, "gs_frame*": C.c_void_p, "float*": C.c_void_p, "int32_t*": C.c_void_p, "gs_stream": C.c_void_p,
             "int32_t": C.c_int32}
    protos = _prototypes()
    for n in NAMES:
        ret, params = protos[n]
        assert ret == "int" and params[-1] == "gs_stream"          # _native.call() appends the stream
        assert n not in _native._STREAMLESS
        fn = getattr(L, n)
        assert fn.restype is C.c_int
        assert list(fn.argtypes) == [kinds[p] for p in params] == channels.ARGTYPES[n], n


def test_refuses_null_arguments_without_a_gpu():
    """argument checks come before anything that needs a device"""
    from taichi_3d_gaussian_splatting_amd import _native, channels
    channels._bind()
    L = _native.lib()
    for n in NAMES:
        assert getattr(L, n)(None, None, None, 3, None, None, None) == -1        # GS_ERR_INVALID_ARGUMENT
        assert b"NULL" in L.gs_last_error()


def test_product_sources_do_not_mention_the_checker():
    for path in (os.path.join(PKG, "channels.py"), os.path.join(PKG, "csrc", "k_channels.hip"), HEADER):
        assert "oracle" not in open(path).read().lower(), path


def test_operator_surface():
    import inspect
    from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast
    assert "keep_frame" in inspect.signature(Rast.forward).parameters
    assert inspect.signature(Rast.forward).parameters["keep_frame"].default is False
    assert list(inspect.signature(Rast.render_channels).parameters) == ["self", "values", "frame"]
