"""CPU: the C ABI of the mixture's gradient calls (include/gs_mixture_grad.h) and their binding (mixture_grad.py, mixture.py)."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gs_mixture_grad.h")
PKG = os.path.join(ROOT, "taichi_3d_gaussian_splatting_amd")
SOURCE = os.path.join(PKG, "csrc", "k_mixture_grad.hip")
NAMES = ["gs_mixture_fourier_backward", "gs_mixture_log_density_backward"]


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
                   '  int (*d)(gs_ctx*, const float*, const float*, const int8_t*, int64_t, const float*, int64_t, const float*, const float*,\n'
                   '           float*, float*, float*, gs_stream) = gs_mixture_log_density_backward;\n'
                   '  int (*f)(gs_ctx*, const float*, const float*, const int8_t*, int64_t, const float*, int64_t, const float*, const float*,\n'
                   '           float*, float*, gs_stream) = gs_mixture_fourier_backward;\n'
                   '  (void)d; (void)f; return GS_MIXTURE_MAX_POINTS > 0 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", str(src), "-o", str(tmp_path / "probe.o")])
    assert sorted(_prototypes()) == NAMES


def test_library_exports_the_symbols_outside_the_versioned_list():
    from taichi_3d_gaussian_splatting_amd import _native
    L = _native.lib()
    for n in NAMES:
        assert hasattr(L, n), f"libgsrast.so does not export {n}"
        assert n not in _native.SYMBOLS
    names = L.gs_kernel_names().decode().split(",")
    assert not any("mix" in n for n in names)


def test_argtypes_match_the_prototypes():
    from taichi_3d_gaussian_splatting_amd import _native, mixture_grad
    mixture_grad._bind()
    L = _native.lib()
    kinds = {"gs_ctx*": C.c_void_p, "float*": C.c_void_p, "int8_t*": C.c_void_p, "gs_stream": C.c_void_p, "int64_t": C.c_int64}
    protos = _prototypes()
    assert sorted(mixture_grad.ARGTYPES) == NAMES
    for name in NAMES:
        ret, params = protos[name]
        assert ret == "int" and params[-1] == "gs_stream"          # _native.call() appends the stream
        assert name not in _native._STREAMLESS
        fn = getattr(L, name)
        assert fn.restype is C.c_int
        assert list(fn.argtypes) == [kinds[p] for p in params] == mixture_grad.ARGTYPES[name]


def _calls(L, p):
    """the two calls over (ctx, point_cloud, features, n_points, queries, n_q, upstream, grad_point_cloud, grad_features)"""
    def density(ctx, pc, feat, n, x, n_x, g, gpc, gfeat, log_p=p, gx=None):
        return L.gs_mixture_log_density_backward(ctx, pc, feat, None, n, x, n_x, log_p, g, gpc, gfeat, gx, None)

    def transform(ctx, pc, feat, n, k, n_k, g, gpc, gfeat, centre=p):
        return L.gs_mixture_fourier_backward(ctx, pc, feat, None, n, k, n_k, centre, g, gpc, gfeat, None)
    return density, transform


def test_refuses_bad_arguments_without_a_gpu():
    """argument checks come before anything that needs a device"""
    from taichi_3d_gaussian_splatting_amd import _native, mixture_grad
    mixture_grad._bind()
    L = _native.lib()
    buf = (C.c_float * 256)()
    p = C.cast(buf, C.c_void_p)
    ctx = C.c_void_p(8)          # a context handle that is never dereferenced: every call below is refused, or found empty, before that
    for call in _calls(L, p):
        assert call(None, p, p, 2, p, 2, p, p, p) == -1                  # GS_ERR_INVALID_ARGUMENT
        assert b"NULL" in L.gs_last_error()
        for n in (-1, 2 ** 30 + 1, 2 ** 31):
            assert call(ctx, p, p, n, p, 2, p, p, p) == -1, n
            assert b"n_points" in L.gs_last_error()
            assert call(ctx, p, p, 2, p, n, p, p, p) == -1, n
            assert b"n_x" in L.gs_last_error() or b"n_k" in L.gs_last_error()
        for hole in range(6):                                            # each required array in turn
            arrays = [p] * 6
            arrays[hole] = None
            pc, feat, q, g, gpc, gfeat = arrays
            assert call(ctx, pc, feat, 2, q, 2, g, gpc, gfeat) == -1, hole
            assert b"NULL" in L.gs_last_error()
        # nothing to do is not an error, with or without pointers
        assert call(ctx, None, None, 0, None, 0, None, None, None) == 0
        assert call(ctx, p, p, 2, None, 0, None, None, None) == 0
        assert call(ctx, None, None, 0, p, 2, p, p, p) == 0
    density, transform = _calls(L, p)
    assert density(ctx, p, p, 2, p, 2, p, p, p, log_p=None) == -1 and b"NULL" in L.gs_last_error()
    assert transform(ctx, p, p, 2, p, 2, p, p, p, centre=None) == -1 and b"NULL" in L.gs_last_error()


def test_blocking_agrees_between_the_kernels_and_python():
    from taichi_3d_gaussian_splatting_amd import mixture, mixture_grad
    src = open(SOURCE).read()
    assert _define(src, "GS_MIXG_COMPONENTS_PER_WG") == mixture_grad.COMPONENTS_PER_WORKGROUP
    assert _define(src, "GS_MIXG_COMPONENTS_PER_WG") == _define(src, "GS_MIXG_LANES") * _define(src, "GS_MIXG_LANE_COMPONENTS")
    assert _define(src, "GS_MIXG_QUERY_CHUNK") == mixture_grad.QUERIES_PER_CHUNK
    assert _define(src, "GS_MIXG_RUN") == mixture_grad.RUN_LENGTH
    assert _define(src, "GS_MIXG_TARGET_WGS") == mixture_grad.TARGET_WORKGROUPS
    assert _define(src, "GS_MIXG_MAX_QUERY_CHUNKS") == mixture_grad.MAX_QUERY_CHUNKS
    assert mixture_grad.N_FEATURES == mixture.N_FEATURES
    # the split of the query loop, restated in Python for the tests: one chunk per unit while the grid is small, never more
    # chunks than units or than the cap
    qc = mixture_grad.QUERIES_PER_CHUNK
    assert mixture_grad.query_chunks(1, 1) == (1, qc) and mixture_grad.query_chunks(1, 2 * qc) == (2, qc)
    assert mixture_grad.query_chunks(1, 2 * qc + 1) == (3, qc)
    assert mixture_grad.query_chunks(1, 1000 * qc)[0] <= mixture_grad.MAX_QUERY_CHUNKS
    assert mixture_grad.query_chunks(10 ** 6, 10 ** 5)[0] == 1


def test_cpu_tensors_are_refused_naming_the_gpu():
    from taichi_3d_gaussian_splatting_amd import mixture, mixture_grad
    pc, feat = torch.zeros(10, 3, requires_grad=True), torch.zeros(10, 56, requires_grad=True)
    scene = (pc, feat, torch.zeros(10, dtype=torch.int8))
    x = torch.zeros(4, 3)
    for fn in (mixture.log_density, mixture.density):
        with pytest.raises(ValueError, match="GPU"):
            fn(scene, x)
    with pytest.raises(ValueError, match="GPU"):
        mixture.fourier(scene, x, torch.zeros(3))
    with pytest.raises(ValueError, match="GPU"):
        mixture_grad.log_density_backward(scene, x, torch.zeros(4), torch.zeros(4))
    with pytest.raises(ValueError, match="GPU"):
        mixture_grad.fourier_backward(scene, x, torch.zeros(3), torch.zeros(4, 2))


def test_a_gradient_to_k_or_centre_is_an_error_that_names_the_argument():
    from taichi_3d_gaussian_splatting_amd import mixture
    scene = (torch.zeros(10, 3), torch.zeros(10, 56), None)
    with pytest.raises(ValueError, match=r"\bk requires a gradient"):
        mixture.fourier(scene, torch.zeros(4, 3, requires_grad=True), torch.zeros(3))
    with pytest.raises(ValueError, match=r"\bcentre requires a gradient"):
        mixture.fourier(scene, torch.zeros(4, 3), torch.zeros(3, requires_grad=True))
    with torch.no_grad(), pytest.raises(ValueError, match="GPU"):        # without grad mode nothing is asked for: the usual refusal
        mixture.fourier(scene, torch.zeros(4, 3, requires_grad=True), torch.zeros(3))


def test_product_sources_do_not_mention_the_checker():
    for path in (os.path.join(PKG, "mixture_grad.py"), SOURCE, HEADER):
        assert "oracle" not in open(path).read().lower(), path
