"""CPU: the C ABI of the packed rows and their merge (include/gs_exchange.h) and their binding (exchange.py)."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gs_exchange.h")
PKG = os.path.join(ROOT, "taichi_3d_gaussian_splatting_amd")
NAMES = ["gs_merge_rows", "gs_pack_rows"]


def _prototypes(header=HEADER):
    src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w ]*?[\w*])\s+(gs_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        types = [re.sub(r"\bconst\b|\s", "", re.match(r"(.*?)(\w+)$", p.strip()).group(1)) for p in params.split(",")]
        protos[name] = (ret.strip(), types)
    return protos


def test_header_is_plain_c99_and_declares_the_two_functions(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(f'#include "{HEADER}"\n'
                   'int main(void) {\n'
                   '  int (*p)(gs_ctx*, const float*, const float*, int64_t, const int32_t*, const int32_t*, int64_t, float*, gs_stream) = gs_pack_rows;\n'
                   '  int (*m)(gs_ctx*, const float*, const int32_t*, int32_t, int64_t, int64_t, float*, float*, int32_t*, int64_t, int32_t*,\n'
                   '           gs_stream) = gs_merge_rows;\n'
                   '  int row[GS_PACKED_ROW_WORDS == 60 && GS_MERGE_MAX_LISTS == 64 ? 1 : -1];\n'
                   '  (void)p; (void)m; (void)row; return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", str(src), "-o", str(tmp_path / "probe.o")])
    assert sorted(_prototypes()) == NAMES


def test_library_exports_both_symbols_and_the_other_headers_are_unchanged():
    from taichi_3d_gaussian_splatting_amd import _native, exchange
    L = _native.lib()
    for n in NAMES:
        assert hasattr(L, n), f"libgsrast.so does not export {n}"
        assert n not in _native.SYMBOLS
    assert L.gs_abi_version() == _native.ABI_VERSION == 9
    assert len(L.gs_kernel_names().decode().split(",")) == 13
    for header in ("gs_rasterizer.h", "gs_sparse.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        for word in ("gs_exchange", "gs_pack", "gs_merge", "packed"):
            assert word not in text and word.upper() not in text, (header, word)
    assert sorted(_prototypes(os.path.join(ROOT, "include", "gs_sparse.h"))) == ["gs_adam_step_rows", "gs_touched_rows"]
    src = open(HEADER).read()
    assert int(re.search(r"#define\s+GS_PACKED_ROW_WORDS\s+(\d+)", src).group(1)) == exchange.ROW_WORDS == 60
    assert int(re.search(r"#define\s+GS_MERGE_MAX_LISTS\s+(\d+)", src).group(1)) == exchange.MAX_LISTS == 64
    assert exchange.ROW_BYTES == 240


def test_argtypes_match_the_prototypes():
    from taichi_3d_gaussian_splatting_amd import _native, exchange
    exchange._bind()
    L = _native.lib()
    kinds = {"gs_ctx*": C.c_void_p, "float*": C.c_void_p, "int32_t*": C.c_void_p, "gs_stream": C.c_void_p,
             "int32_t": C.c_int32, "int64_t": C.c_int64}
    protos = _prototypes()
    for n in NAMES:
        ret, params = protos[n]
        assert ret == "int" and params[-1] == "gs_stream"          # _native.call() appends the stream
        assert n not in _native._STREAMLESS
        fn = getattr(L, n)
        assert fn.restype is C.c_int
        assert list(fn.argtypes) == [kinds[p] for p in params] == exchange.ARGTYPES[n], n


def test_refuses_null_and_bad_arguments_without_a_gpu():
    """argument checks come before anything that needs a device"""
    from taichi_3d_gaussian_splatting_amd import _native, exchange
    exchange._bind()
    L = _native.lib()
    INVALID = -1                                                                 # GS_ERR_INVALID_ARGUMENT
    assert L.gs_pack_rows(None, None, None, 10, None, None, 10, None, None) == INVALID
    assert b"NULL" in L.gs_last_error()
    assert L.gs_merge_rows(None, None, None, 2, 10, 10, None, None, None, 10, None, None) == INVALID
    assert b"NULL" in L.gs_last_error()
    # a context handle that is never dereferenced: these are refused (or found to be empty) before the context is looked at
    ctx = C.c_void_p(8)
    buf = (C.c_float * 64)()
    ids = (C.c_int32 * 4)()
    p, i = C.cast(buf, C.c_void_p), C.cast(ids, C.c_void_p)
    aligned = C.c_void_p((p.value + 15) & ~15)
    assert L.gs_pack_rows(ctx, None, None, 10, None, None, 10, None, None) == INVALID
    assert b"NULL" in L.gs_last_error()
    for n_rows, max_count in ((-1, 10), (10, -1), (2 ** 31, 10)):
        assert L.gs_pack_rows(ctx, p, p, n_rows, i, i, max_count, aligned, None) == INVALID, (n_rows, max_count)
        assert b">= 0" in L.gs_last_error()
    assert L.gs_pack_rows(ctx, p, p, 10, i, i, 10, C.c_void_p(aligned.value + 4), None) == INVALID
    assert b"aligned" in L.gs_last_error()
    # nothing to do is not an error, with or without pointers: no launch when max_count == 0 or n_rows == 0
    assert L.gs_pack_rows(ctx, None, None, 10, None, None, 0, None, None) == 0
    assert L.gs_pack_rows(ctx, None, None, 0, None, None, 10, None, None) == 0
    assert L.gs_pack_rows(ctx, p, p, 0, i, i, 10, aligned, None) == 0

    def merge(n_lists=2, list_stride=4, n_rows=10, capacity=8, packed=aligned, out=p, ints=i, count=i):
        return L.gs_merge_rows(ctx, packed, ints, n_lists, list_stride, n_rows, out, out, ints, capacity, count, None)
    for n_lists in (0, 65, -1):
        assert merge(n_lists=n_lists, capacity=1000) == INVALID, n_lists
        assert b"n_lists" in L.gs_last_error()
    for kw in (dict(list_stride=-1), dict(n_rows=-1), dict(n_rows=2 ** 31 - 4095, capacity=2 ** 31)):
        assert merge(**kw) == INVALID, kw
        assert b">= 0" in L.gs_last_error()
    for kw in (dict(capacity=7), dict(capacity=-1), dict(n_rows=5, capacity=4), dict(n_lists=64, list_stride=1, n_rows=100, capacity=63)):
        assert merge(**kw) == INVALID, kw
        assert b"union_capacity" in L.gs_last_error()
    for kw in (dict(packed=None), dict(out=None), dict(ints=None), dict(count=None)):
        assert merge(**kw) == INVALID, kw
        assert b"NULL" in L.gs_last_error()
    assert merge(packed=C.c_void_p(aligned.value + 4)) == INVALID
    assert b"aligned" in L.gs_last_error()
    # nothing to merge and nowhere to write the empty count: no launch, no error
    assert merge(n_rows=0, capacity=0, count=None) == 0
    assert merge(list_stride=0, capacity=0, count=None) == 0
    assert L.gs_merge_rows(ctx, None, None, 1, 0, 10, None, None, None, 0, None, None) == 0


def test_product_sources_do_not_mention_the_checker():
    for path in (os.path.join(PKG, "exchange.py"), os.path.join(PKG, "csrc", "k_exchange.hip"), HEADER):
        assert "oracle" not in open(path).read().lower(), path


def test_python_surface():
    import inspect
    from taichi_3d_gaussian_splatting_amd import distributed, exchange
    pack = inspect.signature(exchange.pack_rows).parameters
    assert list(pack) == ["grad_pointcloud", "grad_features", "rows", "out"] and pack["out"].default is None
    merge = inspect.signature(exchange.merge_rows).parameters
    assert list(merge) == ["packed", "counts", "n_points", "out", "zero"] and merge["out"].default is None and merge["zero"].default is False
    reduce = inspect.signature(distributed.sparse_reduce_point_gradients).parameters
    assert list(reduce) == ["grad_pc", "grad_feat", "rows", "group", "zero"] and reduce["group"].default is None and reduce["zero"].default is False
    for member in ("data", "count", "n_points", "max_count"):
        assert member in exchange.PackedRows.__slots__
    doc = " ".join(distributed.sparse_reduce_point_gradients.__doc__.split())
    assert "((g0 + g1) + g2)" in doc and "not claimed beyond two ranks" in doc
    src = open(os.path.join(PKG, "csrc", "k_exchange.hip")).read()
    assert int(re.search(r"#define\s+GS_XROW_WORDS\s+(\d+)", src).group(1)) == exchange.ROW_WORDS
    assert "atomic" not in re.sub(r"//.*", "", src)                             # no float or integer atomic in the kernels
