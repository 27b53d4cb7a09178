"""CPU: the C ABI of the touched-row list and the row-selective Adam step (include/gs_sparse.h) and their binding (sparse.py)."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gs_sparse.h")
PKG = os.path.join(ROOT, "taichi_3d_gaussian_splatting_amd")
NAMES = ["gs_adam_step_rows", "gs_touched_rows"]


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w ]*?[\w*])\s+(gs_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        types = [re.sub(r"\bconst\b|\s", "", re.match(r"(.*?)(\w+)$", p.strip()).group(1)) for p in params.split(",")]
        protos[name] = (ret.strip(), types)
    return protos


def test_header_is_plain_c99_and_declares_the_two_functions(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(f'#include "{HEADER}"\n'
                   'int main(void) {\n'
                   '  int (*t)(gs_ctx*, const gs_frame*, int32_t*, int64_t, int32_t*, gs_stream) = gs_touched_rows;\n'
                   '  int (*a)(gs_ctx*, float*, const float*, float*, float*, int64_t, int32_t, const int32_t*, const int32_t*, int64_t,\n'
                   '           float, float, float, float, int64_t, gs_stream) = gs_adam_step_rows;\n'
                   '  (void)t; (void)a; return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", str(src), "-o", str(tmp_path / "probe.o")])
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
    for word in ("gs_sparse", "gs_touched", "gs_adam_step_rows"):
        assert word not in main and word.upper() not in main, word


def test_argtypes_match_the_prototypes():
    from taichi_3d_gaussian_splatting_amd import _native, sparse
    sparse._bind()
    L = _native.lib()
    kinds = {"gs_ctx*": C.c_void_p, "gs_frame*": C.c_void_p, "float*": C.c_void_p, "int32_t*": C.c_void_p, "gs_stream": C.c_void_p,
             "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
    protos = _prototypes()
    for n in NAMES:
        ret, params = protos[n]
        assert ret == "int" and params[-1] == "gs_stream"          # _native.call() appends the stream
        assert n not in _native._STREAMLESS
        fn = getattr(L, n)
        assert fn.restype is C.c_int
        assert list(fn.argtypes) == [kinds[p] for p in params] == sparse.ARGTYPES[n], n


def test_refuses_null_and_bad_arguments_without_a_gpu():
    """argument checks come before anything that needs a device"""
    from taichi_3d_gaussian_splatting_amd import _native, sparse
    sparse._bind()
    L = _native.lib()
    assert L.gs_touched_rows(None, None, None, 10, None, None) == -1             # GS_ERR_INVALID_ARGUMENT
    assert b"NULL" in L.gs_last_error()
    assert L.gs_adam_step_rows(None, None, None, None, None, 10, 56, None, None, 10, 1e-3, 0.9, 0.999, 1e-8, 1, None) == -1
    assert b"NULL" in L.gs_last_error()
    # a context handle that is never dereferenced: these are refused (or found to be empty) before the context is looked at
    ctx = C.c_void_p(8)
    assert L.gs_adam_step_rows(ctx, None, None, None, None, 10, 56, None, None, 10, 1e-3, 0.9, 0.999, 1e-8, 1, None) == -1
    assert b"NULL" in L.gs_last_error()
    buf = (C.c_float * 4)()
    ids = (C.c_int32 * 4)()
    p, i = C.cast(buf, C.c_void_p), C.cast(ids, C.c_void_p)
    for row_len, step, n_rows, max_count in ((0, 1, 10, 10), (56, 0, 10, 10), (56, 1, 10, -1), (56, 1, -1, 10)):
        assert L.gs_adam_step_rows(ctx, p, p, p, p, n_rows, row_len, i, i, max_count, 1e-3, 0.9, 0.999, 1e-8, step, None) == -1, (row_len, step)
        assert b">= " in L.gs_last_error()
    # nothing to do is not an error, with or without pointers: no launch when max_count == 0 (or the tensor is empty)
    assert L.gs_adam_step_rows(ctx, None, None, None, None, 10, 56, None, None, 0, 1e-3, 0.9, 0.999, 1e-8, 1, None) == 0
    assert L.gs_adam_step_rows(ctx, None, None, None, None, 0, 56, None, None, 10, 1e-3, 0.9, 0.999, 1e-8, 1, None) == 0


def test_product_sources_do_not_mention_the_checker():
    for path in (os.path.join(PKG, "sparse.py"), os.path.join(PKG, "csrc", "k_sparse.hip"), HEADER):
        assert "oracle" not in open(path).read().lower(), path


def test_python_surface():
    import inspect
    from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast, sparse
    from taichi_3d_gaussian_splatting_amd.optim import FusedAdam
    step = inspect.signature(FusedAdam.step).parameters
    assert list(step) == ["self", "rows"] and step["rows"].default is None
    assert Rast.track_touched_rows is False
    assert "track_touched_rows" not in getattr(Rast.GaussianPointCloudRasterisationConfig, "__dataclass_fields__")
    assert isinstance(sparse.COMPACT_BLOCK, int) and sparse.COMPACT_BLOCK % 64 == 0
    src = open(os.path.join(PKG, "csrc", "k_sparse.hip")).read()
    assert int(re.search(r"#define\s+GS_ROWS_BLOCK\s+(\d+)", src).group(1)) == sparse.COMPACT_BLOCK
    assert "synchronises" in " ".join(sparse.TouchedRows.tensor.__doc__.lower().split())
    for member in ("ids", "count", "n_points", "max_count"):
        assert member in sparse.TouchedRows.__slots__
