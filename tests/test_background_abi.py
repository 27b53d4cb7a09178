"""CPU: the C ABI of the background (include/gs_background.h) and its binding (background.py)."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gs_background.h")
PKG = os.path.join(ROOT, "taichi_3d_gaussian_splatting_amd")
NAMES = ["gs_background_backward", "gs_background_composite"]
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
                   '  int (*f)(gs_ctx*, const gs_loss_image*, const float*, const float*, int32_t, const float*, const float*, int32_t, int32_t,\n'
                   '           int32_t, const gs_loss_image*, gs_stream) = gs_background_composite;\n'
                   '  int (*g)(gs_ctx*, const gs_loss_image*, const float*, const float*, int32_t, const float*, const float*, int32_t, int32_t,\n'
                   '           float*, float*, gs_stream) = gs_background_backward;\n'
                   '  (void)f; (void)g;\n'
                   '  return GS_BACKGROUND_PIXELS_PER_BLOCK == 1024 && GS_BACKGROUND_COEF_FLOATS == 48 && GS_BACKGROUND_MAX_PIXELS == 2147481600 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", str(src), "-o", str(tmp_path / "probe.o")])
    assert sorted(_prototypes()) == NAMES


def test_library_exports_the_symbols_and_the_main_header_is_unchanged():
    from taichi_3d_gaussian_splatting_amd import _native
    L = _native.lib()
    for n in NAMES:
        assert hasattr(L, n), f"libgsrast.so does not export {n}"
        assert n not in _native.SYMBOLS
    assert L.gs_abi_version() == _native.ABI_VERSION == 9
    assert len(L.gs_kernel_names().decode().split(",")) == 13
    assert "background" not in open(os.path.join(ROOT, "include", "gs_rasterizer.h")).read().lower()


def test_argtypes_match_the_prototypes():
    from taichi_3d_gaussian_splatting_amd import _native, background
    background._bind()
    L = _native.lib()
    kinds = {"gs_ctx*": C.c_void_p, "float*": C.c_void_p, "gs_stream": C.c_void_p, "int32_t": C.c_int32,
             "gs_loss_image*": C.POINTER(_native.GsLossImage)}
    protos = _prototypes()
    assert sorted(background.ARGTYPES) == NAMES
    for name in NAMES:
        ret, params = protos[name]
        assert ret == "int" and params[-1] == "gs_stream"          # _native.call() appends the stream
        assert name not in _native._STREAMLESS
        fn = getattr(L, name)
        assert fn.restype is C.c_int
        assert list(fn.argtypes) == [kinds[p] for p in params] == background.ARGTYPES[name], name


def test_macros_agree_between_the_header_python_and_the_reference():
    from taichi_3d_gaussian_splatting_amd import background
    import background_ref
    assert _define("GS_BACKGROUND_PIXELS_PER_BLOCK") == background.PIXELS_PER_BLOCK == background_ref.PIXELS_PER_BLOCK == 1024
    assert _define("GS_BACKGROUND_FINISH_THREADS") == background.FINISH_THREADS == background_ref.FINISH_THREADS == 256
    assert _define("GS_BACKGROUND_FINISH_BLOCKS") == background.FINISH_BLOCKS == background_ref.FINISH_BLOCKS == 48
    assert _define("GS_BACKGROUND_COEF_FLOATS") == background.COEF_FLOATS == background_ref.COEF_FLOATS == 48 == 3 * 16
    assert _define("GS_BACKGROUND_MAX_BANDS") == background.MAX_BANDS == background_ref.MAX_BANDS == 3
    assert _define("GS_BACKGROUND_MAX_PIXELS") == background.MAX_PIXELS == 2 ** 31 - 2048
    assert _define("GS_BACKGROUND_STRAIGHT") == background.STRAIGHT == background_ref.STRAIGHT == 1
    assert _define("GS_BACKGROUND_COLOURS_ONLY") == background.COLOURS_ONLY == background_ref.COLOURS_ONLY == 2
    # a 1920x1088 frame has more per-block sums than a finishing block has threads: its loop runs
    assert 1920 * 1088 // background.PIXELS_PER_BLOCK > background.FINISH_THREADS


def _image(buf, **over):
    from taichi_3d_gaussian_splatting_amd import _native
    f = dict(data=C.cast(buf, C.c_void_p).value, stride_channel=16, stride_row=4, stride_column=1)
    f.update(over)
    return _native.GsLossImage(**f)


def test_bad_arguments_are_refused_without_a_gpu():
    """argument checks come before anything that needs a device"""
    from taichi_3d_gaussian_splatting_amd import _native, background
    background._bind()
    L = _native.lib()
    composite, backward, err = L.gs_background_composite, L.gs_background_backward, L.gs_last_error
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    im, no_data = _image(buf), _image(buf, data=None)
    H = W = 4
    assert composite(None, im, p, p, 0, None, None, H, W, 0, im, None) == INVALID and b"ctx is NULL" in err()
    assert backward(None, im, p, p, 0, None, None, H, W, p, p, None) == INVALID and b"ctx is NULL" in err()
    ctx = C.c_void_p(8)       # a context handle that is never dereferenced: everything below is refused before it is looked at
    for bad in (None, no_data):
        assert composite(ctx, bad, p, p, 0, None, None, H, W, 0, im, None) == INVALID and b"NULL image" in err()
        assert composite(ctx, bad, p, p, 0, None, None, H, W, background.STRAIGHT, im, None) == INVALID and b"NULL image" in err()
        assert composite(ctx, im, p, p, 0, None, None, H, W, 0, bad, None) == INVALID and b"NULL out" in err()
        assert composite(ctx, None, None, p, 0, None, None, H, W, background.COLOURS_ONLY, bad, None) == INVALID and b"NULL out" in err()
        assert backward(ctx, bad, p, p, 0, None, None, H, W, p, p, None) == INVALID and b"NULL grad_out" in err()
    assert composite(ctx, im, None, p, 0, None, None, H, W, 0, im, None) == INVALID and b"alpha is NULL" in err()
    assert backward(ctx, im, None, p, 0, None, None, H, W, p, p, None) == INVALID and b"alpha is NULL" in err()
    assert composite(ctx, im, p, None, 0, None, None, H, W, 0, im, None) == INVALID and b"coef is NULL" in err()
    assert backward(ctx, im, p, None, 0, None, None, H, W, p, p, None) == INVALID and b"coef is NULL" in err()
    assert backward(ctx, im, p, p, 0, None, None, H, W, None, None, None) == INVALID and b"both NULL" in err()
    # the new cases: bands outside 0..3, and a sky without its camera
    for bands in (-1, 4, 16):
        assert composite(ctx, im, p, p, bands, p, p, H, W, 0, im, None) == INVALID and b"bands must be 0 .. 3" in err()
        assert backward(ctx, im, p, p, bands, p, p, H, W, p, p, None) == INVALID and b"bands must be 0 .. 3" in err()
    for bands in (1, 2, 3):
        for q, k in ((None, p), (p, None), (None, None)):
            assert composite(ctx, im, p, p, bands, q, k, H, W, 0, im, None) == INVALID and b"needs q and intrinsics" in err()
            assert composite(ctx, None, None, p, bands, q, k, H, W, background.COLOURS_ONLY, im, None) == INVALID and b"needs q and" in err()
            assert backward(ctx, im, p, p, bands, q, k, H, W, p, p, None) == INVALID and b"needs q and intrinsics" in err()
    for flags in (3, 4, -1):
        assert composite(ctx, im, p, p, 0, None, None, H, W, flags, im, None) == INVALID and b"flags" in err()
    for h, w in ((0, 4), (4, 0), (-1, 4), (4, -3)):
        assert composite(ctx, im, p, p, 0, None, None, h, w, 0, im, None) == INVALID and b">= 1" in err()
        assert backward(ctx, im, p, p, 0, None, None, h, w, p, p, None) == INVALID and b">= 1" in err()
    assert composite(ctx, im, p, p, 0, None, None, 2 ** 16, 2 ** 15, 0, im, None) == INVALID and b"too many pixels" in err()
    assert backward(ctx, im, p, p, 0, None, None, 2 ** 16, 2 ** 15, p, p, None) == INVALID and b"too many pixels" in err()


def test_cpu_tensors_wrong_dtypes_and_shapes_are_refused_in_python():
    from taichi_3d_gaussian_splatting_amd import background
    image, alpha, coef = torch.zeros(3, 4, 5), torch.zeros(4, 5), torch.zeros(48)
    for call in (lambda: background.composite(image, alpha, coef, 0), lambda: background.composite_forward(image, alpha, coef, 0),
                 lambda: background.composite_backward(image, alpha, coef, 0), lambda: background.colours(coef, 0, None, None, 4, 5),
                 lambda: background.composite_straight(torch.zeros(4, 4, 5), coef, 0)):
        with pytest.raises(ValueError, match="GPU"):
            call()
    with pytest.raises(ValueError, match="GPU"):
        background.BackgroundModel("sky", "cpu")
    with pytest.raises(ValueError, match="kind"):
        background.BackgroundModel("none", "cpu")
    with pytest.raises(TypeError, match="float32"):
        background.composite(image.double(), alpha, coef, 0)
    with pytest.raises(TypeError, match="tensor"):
        background.composite(image.numpy(), alpha, coef, 0)
    for bad in (torch.zeros(4, 4, 5), torch.zeros(3, 4), torch.zeros(3, 0, 5)):
        with pytest.raises(ValueError, match=r"\(3,H,W\)"):
            background.composite(bad, alpha, coef, 0)
    with pytest.raises(ValueError, match=r"\(4,H,W\)"):
        background.composite_straight(torch.zeros(3, 4, 5), coef, 0)

    # the checks behind the device test, against tensors that are on no CPU
    meta = torch.device("meta")
    fake_coef, fake_q, fake_k = torch.zeros(48, device=meta), torch.zeros(1, 4, device=meta), torch.zeros(3, 3, device=meta)
    background.check_background(fake_coef, 3, fake_q, fake_k, meta)
    background.check_background(fake_coef, 0, None, None, meta)
    for bands in (-1, 4, 1.0, True):
        with pytest.raises(ValueError, match="bands"):
            background.check_background(fake_coef, bands, fake_q, fake_k, meta)
    for q, k in ((None, fake_k), (fake_q, None)):
        with pytest.raises(ValueError, match="needs q"):
            background.check_background(fake_coef, 2, q, k, meta)
    for name, args, exc in (("coef", (torch.zeros(16, device=meta), 0, None, None), ValueError),
                            ("coef", (torch.zeros(48, dtype=torch.float64, device=meta), 0, None, None), TypeError),
                            ("coef", (torch.zeros(96, device=meta)[::2], 0, None, None), ValueError),
                            ("coef", (torch.zeros(48), 0, None, None), ValueError),
                            ("q", (fake_coef, 1, torch.zeros(3, device=meta), fake_k), ValueError),
                            ("intrinsics", (fake_coef, 1, fake_q, torch.zeros(3, 4, device=meta)), ValueError)):
        with pytest.raises(exc, match=name):
            background.check_background(*args, meta)
    for bad, exc in ((torch.zeros(5, 4, device=meta), ValueError), (torch.zeros(4, 5, dtype=torch.float16, device=meta), TypeError),
                     (torch.zeros(4, 10, device=meta)[:, ::2], ValueError), (torch.zeros(4, 5), ValueError), (None, TypeError)):
        with pytest.raises(exc, match="alpha"):
            background.check_plane(bad, (4, 5), meta)
    for bad in (dict(lr=0.0), dict(lr_final=float("nan")), dict(num_iterations=0), dict(betas=(1.0, 0.999)), dict(eps=0.0), dict(bands=4),
                dict(bands=-1), dict(colour=(0.0, 1.0)), dict(colour=(0.0, float("inf"), 0.0))):
        with pytest.raises(ValueError):
            background.BackgroundConfig(**bad).check()
    config = background.BackgroundConfig()
    assert (tuple(config.colour), config.bands, config.lr, config.lr_final, config.num_iterations, config.seed) == ((0, 0, 0), 2, 0.01, 0.001, None, 0)
    assert background.colour_coefficients((1.0, 0.5, 0.25), "cpu").tolist() == [1.0] + [0.0] * 15 + [0.5] + [0.0] * 15 + [0.25] + [0.0] * 15


def test_trainer_and_renderer_take_the_switch_and_the_config_keeps_its_fields():
    import dataclasses
    import inspect
    from taichi_3d_gaussian_splatting_amd.GaussianPointRenderer import GaussianPointRenderer
    from taichi_3d_gaussian_splatting_amd.GaussianPointTrainer import GaussianPointCloudTrainer
    params = inspect.signature(GaussianPointCloudTrainer.__init__).parameters
    assert params["background"].default == "none" and params["background_config"].default is None
    assert params["composite_targets"].default is False
    assert not any("background" in f.name or "composite" in f.name for f in dataclasses.fields(GaussianPointCloudTrainer.TrainConfig))
    assert inspect.signature(GaussianPointRenderer.render).parameters["background"].default is None
    assert inspect.signature(GaussianPointRenderer.run).parameters["background"].default is None


def test_product_sources_do_not_mention_the_checker():
    for path in (os.path.join(PKG, "background.py"), os.path.join(PKG, "csrc", "k_background.hip"), HEADER):
        assert "oracle" not in open(path).read().lower(), path
