"""CPU: the C ABI of the Gaussian normals and their consistency loss (include/gs_normals.h), its binding (normals.py) and the
argument checks that come before any device."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gs_normals.h")
NAMES = ["gs_gaussian_normals_backward", "gs_gaussian_normals_forward", "gs_normal_consistency_backward", "gs_normal_consistency_forward"]
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


def test_header_is_plain_c99_and_declares_the_functions(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(f'#include "{HEADER}"\n'
                   'int main(void) {\n'
                   '  int (*a)(gs_ctx*, const float*, const float*, const int32_t*, const float*, const float*, int64_t, int32_t, float*,\n'
                   '           gs_stream) = gs_gaussian_normals_forward;\n'
                   '  int (*b)(gs_ctx*, const float*, const float*, const int32_t*, const float*, const float*, int64_t, int32_t, const float*,\n'
                   '           float*, gs_stream) = gs_gaussian_normals_backward;\n'
                   '  int (*c)(gs_ctx*, const float*, const float*, const float*, int32_t, int32_t, float, float, float, float, float, float,\n'
                   '           float*, gs_stream) = gs_normal_consistency_forward;\n'
                   '  int (*d)(gs_ctx*, const float*, const float*, const float*, int32_t, int32_t, float, float, float, float, float, float,\n'
                   '           const float*, const float*, float*, float*, gs_stream) = gs_normal_consistency_backward;\n'
                   '  (void)a; (void)b; (void)c; (void)d;\n'
                   '  return GS_NORMALS_FEATURES == 56 && GS_NORMALS_LOSS_TERMS == GS_GEOM_LOSS_TERMS ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", str(src), "-o", str(tmp_path / "probe.o")])
    assert sorted(_prototypes()) == NAMES


def test_library_exports_the_symbols_and_the_main_header_is_unchanged():
    from taichi_3d_gaussian_splatting_amd import _native
    L = _native.lib()
    for n in NAMES:
        assert hasattr(L, n), f"libgsrast.so does not export {n}"
        assert n not in _native.SYMBOLS
    assert L.gs_abi_version() == _native.ABI_VERSION == 9
    main = open(os.path.join(ROOT, "include", "gs_rasterizer.h")).read().lower()
    assert "gs_normals" not in main and "gs_gaussian_normals" not in main and "gs_normal_consistency" not in main


def test_argtypes_match_the_prototypes():
    from taichi_3d_gaussian_splatting_amd import _native, normals
    normals._bind()
    L = _native.lib()
    kinds = {"gs_ctx*": C.c_void_p, "float*": C.c_void_p, "int32_t*": C.c_void_p, "gs_stream": C.c_void_p, "int32_t": C.c_int32,
             "int64_t": C.c_int64, "float": C.c_float}
    protos = _prototypes()
    assert sorted(normals.ARGTYPES) == NAMES
    for name in NAMES:
        ret, params = protos[name]
        assert ret == "int" and params[-1] == "gs_stream"          # _native.call() appends the stream
        assert name not in _native._STREAMLESS
        fn = getattr(L, name)
        assert fn.restype is C.c_int
        assert list(fn.argtypes) == [kinds[p] for p in params] == normals.ARGTYPES[name], name


def test_macros_agree_between_the_header_python_and_the_reference():
    from taichi_3d_gaussian_splatting_amd import geometry, normals
    import normals_ref
    assert _define("GS_NORMALS_FEATURES") == normals.FEATURES == normals_ref.FEATURES == 56
    assert _define("GS_NORMALS_BLOCK") == normals.BLOCK == normals_ref.BLOCK == 256
    assert _define("GS_NORMALS_MAX_PIXELS") == normals.MAX_PIXELS == normals_ref.MAX_PIXELS
    assert 3 * normals.MAX_PIXELS + 3 * geometry.TILE_W < 2 ** 31
    assert _define("GS_NORMALS_LOSS_TERMS") == geometry.LOSS_TERMS == normals_ref.LOSS_TERMS == 8
    assert (_define("GS_NORMALS_FORWARD_LAUNCHES"), _define("GS_NORMALS_BACKWARD_LAUNCHES")) == \
        (normals.FORWARD_LAUNCHES, normals.BACKWARD_LAUNCHES) == (normals_ref.FORWARD_LAUNCHES, normals_ref.BACKWARD_LAUNCHES) == (2, 1)


def test_bad_arguments_are_refused_without_a_gpu():
    """argument checks come before anything that needs a device"""
    from taichi_3d_gaussian_splatting_amd import _native, normals
    normals._bind()
    L = _native.lib()
    gf, gb, cf, cb, err = (L.gs_gaussian_normals_forward, L.gs_gaussian_normals_backward, L.gs_normal_consistency_forward,
                           L.gs_normal_consistency_backward, L.gs_last_error)
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    H = W = 4
    cam = (50.0, 50.0, 2.0, 2.0)
    nan, inf = float("nan"), float("inf")

    def consistency(ctx, h=H, w=W, cam=cam, jump=0.1, min_length=0.5):
        return [cf(ctx, p, p, None, h, w, *cam, jump, min_length, p, None), cb(ctx, p, p, None, h, w, *cam, jump, min_length, p, None, p, p, None)]

    assert consistency(None) == [INVALID] * 2 and b"ctx is NULL" in err()
    assert gf(None, p, p, None, p, p, 4, 1, p, None) == INVALID and b"ctx is NULL" in err()
    assert gb(None, p, p, None, p, p, 4, 1, p, p, None) == INVALID and b"ctx is NULL" in err()
    ctx = C.c_void_p(8)       # a context handle that is never dereferenced: everything below is refused before it is looked at
    # the per-row calls
    for n in (-1, 2 ** 31 - 255, 2 ** 40):
        assert gf(ctx, p, p, None, p, p, n, 1, p, None) == INVALID and b"N must be" in err()
        assert gb(ctx, p, p, None, p, p, n, 1, p, p, None) == INVALID and b"N must be" in err()
    for k in (0, -3):
        assert gf(ctx, p, p, None, p, p, 4, k, p, None) == INVALID and b"K must be" in err()
        assert gb(ctx, p, p, None, p, p, 4, k, p, p, None) == INVALID and b"K must be" in err()
    for i in (0, 1, 3, 4, 7):               # every array but the ids
        args = [p, p, None, p, p, 4, 1, p]
        args[i] = None
        assert gf(ctx, *args, None) == INVALID and b"NULL" in err()
    assert gb(ctx, p, p, None, p, p, 4, 1, None, p, None) == INVALID and b"NULL" in err()
    assert gb(ctx, p, p, None, p, p, 4, 1, p, None, None) == INVALID and b"NULL" in err()
    # the consistency calls: planes, terms, outputs
    assert cf(ctx, None, p, None, H, W, *cam, 0.1, 0.5, p, None) == INVALID and b"D is NULL" in err()
    assert cf(ctx, p, None, None, H, W, *cam, 0.1, 0.5, p, None) == INVALID and b"R is NULL" in err()
    assert cf(ctx, p, p, None, H, W, *cam, 0.1, 0.5, None, None) == INVALID and b"terms is NULL" in err()
    assert cb(ctx, p, p, None, H, W, *cam, 0.1, 0.5, None, None, p, p, None) == INVALID and b"terms is NULL" in err()
    assert cb(ctx, p, p, None, H, W, *cam, 0.1, 0.5, p, None, None, p, None) == INVALID and b"grad_D or grad_R is NULL" in err()
    assert cb(ctx, p, p, None, H, W, *cam, 0.1, 0.5, p, None, p, None, None) == INVALID and b"grad_D or grad_R is NULL" in err()
    for h, w in ((0, 4), (4, 0), (-1, 4), (4, -3)):
        assert consistency(ctx, h=h, w=w) == [INVALID] * 2 and b">= 1" in err()
    assert consistency(ctx, h=2 ** 15, w=2 ** 15) == [INVALID] * 2 and b"too many pixels" in err()
    for bad in ((0.0, 50.0, 2.0, 2.0), (50.0, -1.0, 2.0, 2.0), (nan, 50.0, 2.0, 2.0), (50.0, inf, 2.0, 2.0)):
        assert consistency(ctx, cam=bad) == [INVALID] * 2 and b"fx and fy" in err()
    for bad in ((50.0, 50.0, nan, 2.0), (50.0, 50.0, 2.0, -inf)):
        assert consistency(ctx, cam=bad) == [INVALID] * 2 and b"cx and cy" in err()
    for bad in (-0.1, nan, inf):
        assert consistency(ctx, jump=bad) == [INVALID] * 2 and b"max_rel_jump" in err()
    for bad in (0.0, -0.5, nan, inf):
        assert consistency(ctx, min_length=bad) == [INVALID] * 2 and b"min_length" in err()


def test_cpu_tensors_wrong_dtypes_and_shapes_are_refused_in_python():
    from taichi_3d_gaussian_splatting_amd import normals
    depth, rendered, cam = torch.ones(4, 5), torch.ones(4, 5, 3), (50.0, 50.0, 2.5, 2.0)
    pc, feat, q, t = torch.zeros(6, 3), torch.zeros(6, 56), torch.tensor([[0.0, 0.0, 0.0, 1.0]]), torch.zeros(1, 3)
    for call in (lambda: normals.normal_consistency(depth, rendered, cam), lambda: normals.normal_consistency_forward(depth, rendered, cam),
                 lambda: normals.normal_consistency_backward(depth, rendered, cam, None, 0.1, 0.5, torch.zeros(8)),
                 lambda: normals.gaussian_normals(pc, feat, q, t), lambda: normals.gaussian_normals_forward(pc, feat, q, t),
                 lambda: normals.gaussian_normals_backward(pc, feat, q, t, None, pc)):
        with pytest.raises(ValueError, match="GPU"):
            call()
    # what is wrong with a tensor or a scalar is found before a device is looked at
    with pytest.raises(TypeError, match="float32"):
        normals.normal_consistency(depth.double(), rendered, cam)
    with pytest.raises(ValueError, match=r"rendered_normals must be \(H,W,3\)"):
        normals.normal_consistency(depth, torch.ones(3, 4, 5), cam)               # the planar layout of a prior is not the blend's
    with pytest.raises(TypeError, match="rendered_normals must be float32"):
        normals.normal_consistency(depth, rendered.half(), cam)
    with pytest.raises(ValueError, match="pixel_weight must have the depth's shape"):
        normals.normal_consistency(depth, rendered, cam, torch.ones(5, 4))
    with pytest.raises(ValueError, match="contiguous"):
        normals.normal_consistency(depth, torch.ones(4, 3, 5).permute(0, 2, 1), cam)
    with pytest.raises(ValueError, match="min_length must be finite and > 0"):
        normals.normal_consistency(depth, rendered, cam, min_length=0.0)
    with pytest.raises(ValueError, match="max_rel_jump"):
        normals.normal_consistency(depth, rendered, cam, max_rel_jump=-1.0)
    with pytest.raises(ValueError, match="fx and fy"):
        normals.normal_consistency(depth, rendered, (0.0, 1.0, 0.0, 0.0))
    with pytest.raises(ValueError, match=r"features must have shape \(6,56\)"):
        normals.gaussian_normals(pc, torch.zeros(6, 55), q, t)
    with pytest.raises(ValueError, match=r"t_pointcloud_camera must have shape \(1,3\)"):
        normals.gaussian_normals(pc, feat, q, torch.zeros(2, 3))
    with pytest.raises(TypeError, match="point_object_id must be torch.int32"):
        normals.gaussian_normals(pc, feat, q, t, torch.zeros(6, dtype=torch.int64))
    with pytest.raises(ValueError, match="at least one pose"):
        normals.gaussian_normals(pc, feat, torch.zeros(0, 4), torch.zeros(0, 3))
    with pytest.raises(TypeError, match="tensor"):
        normals.gaussian_normals(pc.numpy(), feat, q, t)
    with pytest.raises(ValueError, match="pose must be"):
        normals.rendered_normals(None, (pc, feat), q)
    with pytest.raises(ValueError, match="scene_or_tensors"):
        normals.rendered_normals(None, (pc,), (q, t))
