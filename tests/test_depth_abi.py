"""CPU: the C ABI of depth supervision (include/gs_depth.h), its binding (depth.py), the dataset's depth files and the trainer's
switch."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gs_depth.h")
PKG = os.path.join(ROOT, "taichi_3d_gaussian_splatting_amd")
NAMES = ["gs_depth_loss_backward", "gs_depth_loss_forward", "gs_depth_resample"]
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
                   '  int (*f)(gs_ctx*, const void*, int32_t, int32_t, int32_t, int64_t, float, int32_t, int32_t, int32_t, int32_t, float, float*,\n'
                   '           gs_stream) = gs_depth_resample;\n'
                   '  int (*g)(gs_ctx*, const float*, const float*, const float*, const float*, int32_t, int32_t, int32_t, float*, gs_stream) =\n'
                   '      gs_depth_loss_forward;\n'
                   '  int (*h)(gs_ctx*, const float*, const float*, const float*, const float*, int32_t, int32_t, int32_t, const float*, const float*,\n'
                   '           float*, gs_stream) = gs_depth_loss_backward;\n'
                   '  (void)f; (void)g; (void)h;\n'
                   '  return GS_DEPTH_PIXELS_PER_BLOCK == 1024 && GS_DEPTH_LOSS_TERMS == 8 && GS_DEPTH_FLAGS_ALL == 15 ? 0 : 1; }\n')
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
    assert "gs_depth_" not in open(os.path.join(ROOT, "include", "gs_rasterizer.h")).read().lower()


def test_argtypes_match_the_prototypes():
    from taichi_3d_gaussian_splatting_amd import _native, depth
    depth._bind()
    L = _native.lib()
    kinds = {"gs_ctx*": C.c_void_p, "void*": C.c_void_p, "float*": C.c_void_p, "gs_stream": C.c_void_p, "int32_t": C.c_int32,
             "int64_t": C.c_int64, "float": C.c_float}
    protos = _prototypes()
    assert sorted(depth.ARGTYPES) == NAMES
    for name in NAMES:
        ret, params = protos[name]
        assert ret == "int" and params[-1] == "gs_stream"          # _native.call() appends the stream
        assert name not in _native._STREAMLESS
        fn = getattr(L, name)
        assert fn.restype is C.c_int
        assert list(fn.argtypes) == [kinds[p] for p in params] == depth.ARGTYPES[name], name


def test_macros_agree_between_the_header_python_and_the_reference():
    from taichi_3d_gaussian_splatting_amd import appearance, depth, targets
    import depth_ref
    assert _define("GS_DEPTH_U16") == depth.FORMAT_U16 == depth_ref.FORMAT_U16 == 0
    assert _define("GS_DEPTH_F32") == depth.FORMAT_F32 == depth_ref.FORMAT_F32 == 1
    assert _define("GS_DEPTH_INVERT_PREDICTED") == depth.INVERT_PREDICTED == depth_ref.INVERT_PREDICTED == 1
    assert _define("GS_DEPTH_INVERT_TARGET") == depth.INVERT_TARGET == depth_ref.INVERT_TARGET == 2
    assert _define("GS_DEPTH_L2") == depth.L2 == depth_ref.L2 == 4
    assert _define("GS_DEPTH_ALIGN") == depth.ALIGN == depth_ref.ALIGN == 8
    assert _define("GS_DEPTH_FLAGS_ALL") == depth.FLAGS_ALL == depth_ref.FLAGS_ALL == 1 | 2 | 4 | 8
    assert _define("GS_DEPTH_PIXELS_PER_BLOCK") == depth.PIXELS_PER_BLOCK == depth_ref.PIXELS_PER_BLOCK == 1024
    assert _define("GS_DEPTH_FINISH_THREADS") == depth.FINISH_THREADS == depth_ref.FINISH_THREADS == 256
    assert _define("GS_DEPTH_MOMENTS") == depth.MOMENTS == depth_ref.MOMENTS == 5
    assert _define("GS_DEPTH_LOSS_TERMS") == depth.LOSS_TERMS == depth_ref.LOSS_TERMS == 8
    assert (_define("GS_DEPTH_FORWARD_LAUNCHES"), _define("GS_DEPTH_FORWARD_LAUNCHES_ALIGN"), _define("GS_DEPTH_BACKWARD_LAUNCHES")) == \
        (depth.FORWARD_LAUNCHES, depth.FORWARD_LAUNCHES_ALIGN, depth.BACKWARD_LAUNCHES) == (2, 4, 1)
    assert depth.MAX_PIXELS == appearance.MAX_PIXELS == 2 ** 31 - 2048
    assert depth.ROW_PITCH_ALIGN == targets.ROW_PITCH_ALIGN == 16
    # the GPU test's largest size has more per-block sums than a finishing block has threads: both loops run
    assert 520 * 512 // depth.PIXELS_PER_BLOCK > depth.FINISH_THREADS
    assert depth.loss_flags("inverse", "l1") == 3 and depth.loss_flags("depth", "l2") == 4
    assert depth.loss_flags("inverse", "l1", align=True, target_is_inverse=True) == 9


def test_bad_arguments_are_refused_without_a_gpu():
    """argument checks come before anything that needs a device"""
    from taichi_3d_gaussian_splatting_amd import _native, depth
    depth._bind()
    L = _native.lib()
    resample, forward, backward, err = L.gs_depth_resample, L.gs_depth_loss_forward, L.gs_depth_loss_backward, L.gs_last_error
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    H = W = 4
    nan, inf = float("nan"), float("inf")
    assert resample(None, p, 0, 8, 8, 16, 1.0, 8, 8, 8, 8, 0.5, p, None) == INVALID and b"ctx is NULL" in err()
    assert forward(None, p, p, p, None, H, W, 0, p, None) == INVALID and b"ctx is NULL" in err()
    assert backward(None, p, p, p, None, H, W, 0, p, None, p, None) == INVALID and b"ctx is NULL" in err()
    ctx = C.c_void_p(8)       # a context handle that is never dereferenced: everything below is refused before it is looked at
    # the loss: planes, terms, sizes, flags
    for k in range(3):
        planes = [p, p, p]
        planes[k] = None
        assert forward(ctx, *planes, None, H, W, 0, p, None) == INVALID and b"NULL plane" in err()
        assert backward(ctx, *planes, None, H, W, 0, p, None, p, None) == INVALID and b"NULL plane" in err()
    assert forward(ctx, p, p, p, p, H, W, 0, None, None) == INVALID and b"loss_terms is NULL" in err()
    assert backward(ctx, p, p, p, p, H, W, 0, None, None, p, None) == INVALID and b"loss_terms is NULL" in err()
    assert backward(ctx, p, p, p, p, H, W, 0, p, None, None, None) == INVALID and b"grad_D is NULL" in err()
    for h, w in ((0, 4), (4, 0), (-1, 4), (4, -3)):
        assert forward(ctx, p, p, p, None, h, w, 0, p, None) == INVALID and b">= 1" in err()
        assert backward(ctx, p, p, p, None, h, w, 0, p, None, p, None) == INVALID and b">= 1" in err()
    assert forward(ctx, p, p, p, None, 2 ** 16, 2 ** 15, 0, p, None) == INVALID and b"too many pixels" in err()
    assert backward(ctx, p, p, p, None, 2 ** 16, 2 ** 15, 0, p, None, p, None) == INVALID and b"too many pixels" in err()
    for flags in (16, 32, -1, 1 << 20):
        assert forward(ctx, p, p, p, None, H, W, flags, p, None) == INVALID and b"unknown flag bits" in err()
        assert backward(ctx, p, p, p, None, H, W, flags, p, None, p, None) == INVALID and b"unknown flag bits" in err()
    # the resample: format, min_coverage, depth_scale, geometry
    assert resample(ctx, p, 2, 8, 8, 16, 1.0, 8, 8, 8, 8, 0.5, p, None) == INVALID and b"unknown src_format" in err()
    for bad in (-0.01, 1.01, nan, inf):
        assert resample(ctx, p, 0, 8, 8, 16, 1.0, 8, 8, 8, 8, bad, p, None) == INVALID and b"min_coverage" in err()
    for bad in (0.0, -1.0, nan, inf):
        assert resample(ctx, p, 0, 8, 8, 16, bad, 8, 8, 8, 8, 0.5, p, None) == INVALID and b"depth_scale" in err()
    assert resample(ctx, p, 0, -1, 8, 16, 1.0, 8, 8, 8, 8, 0.5, p, None) == INVALID and b"every size" in err()
    assert resample(ctx, p, 0, 8, 40000, 80000, 1.0, 8, 8, 8, 8, 0.5, p, None) == INVALID and b"every size" in err()
    assert resample(ctx, p, 0, 8, 8, 16, 1.0, 8, 8, 9, 8, 0.5, p, None) == INVALID and b"crop" in err()
    assert resample(ctx, p, 0, 8, 8, 15, 1.0, 8, 8, 8, 8, 0.5, p, None) == INVALID and b"src_row_pitch_bytes" in err()
    assert resample(ctx, p, 1, 8, 8, 48, 1.0, 8, 8, 8, 8, 0.5, p, None) == INVALID and b"src_row_pitch_bytes" in err()
    assert resample(ctx, None, 0, 8, 8, 16, 1.0, 8, 8, 8, 8, 0.5, p, None) == INVALID and b"NULL src or dst" in err()
    assert resample(ctx, p, 0, 8, 8, 16, 1.0, 8, 8, 8, 8, 0.5, None, None) == INVALID and b"NULL src or dst" in err()
    assert resample(ctx, p, 0, 8, 8, 16, 1.0, 16, 8, 8, 8, 0.5, p, None) == INVALID and b"scale" in err()        # upscaling
    assert resample(ctx, p, 0, 90, 8, 16, 1.0, 10, 8, 8, 8, 0.5, p, None) == INVALID and b"scale" in err()       # beyond 8
    assert resample(ctx, p, 0, 8, 8, 16, 1.0, 8, 8, 0, 8, 0.5, p, None) == 0                                      # nothing to do


def test_cpu_tensors_wrong_dtypes_and_shapes_are_refused_in_python():
    from taichi_3d_gaussian_splatting_amd import depth
    plane = torch.ones(4, 5)
    for call in (lambda: depth.depth_loss(plane, plane, plane), lambda: depth.depth_loss(plane, plane, plane, plane, align=True),
                 lambda: depth.depth_loss_forward(plane, plane, plane), lambda: depth.depth_loss_backward(plane, plane, plane, None, 0, torch.zeros(8)),
                 lambda: depth.depth_resample(plane, (4, 5)), lambda: depth.depth_resample(torch.zeros(4, 5, dtype=torch.uint16), (4, 5))):
        with pytest.raises(ValueError, match="GPU"):
            call()
    with pytest.raises(ValueError, match="GPU"):
        depth.DepthStore([], [], [], "cpu")
    # what is wrong with a tensor is found before its device is looked at
    with pytest.raises(TypeError, match="float32"):
        depth.depth_loss(plane.double(), plane, plane)
    with pytest.raises(TypeError, match="tensor"):
        depth.depth_loss(plane.numpy(), plane, plane)
    with pytest.raises(TypeError, match="target_weight"):
        depth.depth_loss(plane, plane, plane.half())
    for bad in (torch.zeros(3, 4, 5), torch.zeros(4), torch.zeros(0, 5)):
        with pytest.raises(ValueError, match=r"\(H,W\)"):
            depth.depth_loss(bad, plane, plane)
    with pytest.raises(ValueError, match="target must have the depth's shape"):
        depth.depth_loss(plane, torch.ones(5, 4), plane)
    with pytest.raises(ValueError, match="pixel_weight must be contiguous"):
        depth.depth_loss(plane, plane, plane, torch.ones(4, 10)[:, ::2])
    with pytest.raises(TypeError, match="uint16 or float32"):
        depth.depth_resample(torch.zeros(4, 5, dtype=torch.int32), (4, 5))
    with pytest.raises(ValueError, match=r"\(H,W\)"):
        depth.depth_resample(torch.zeros(3, 4, 5), (4, 5))
    for kw in (dict(space="log"), dict(norm="huber")):
        with pytest.raises(ValueError, match=list(kw)[0]):
            depth.depth_loss(plane, plane, plane, **kw)
    with pytest.raises(ValueError, match="inverse"):
        depth.loss_flags("depth", "l1", True, target_is_inverse=True)
    with pytest.raises(ValueError, match="flag"):
        depth.depth_loss_forward(plane, plane, plane, flags=16)
    fake = torch.zeros(4, 5, device="meta")
    for bad in (dict(depth_scale=0.0), dict(depth_scale=float("nan")), dict(min_coverage=1.5), dict(min_coverage=-0.1)):
        with pytest.raises(ValueError, match=list(bad)[0]):
            depth.depth_resample(fake, (4, 5), **bad)

    for bad in (dict(space="log"), dict(norm="l3"), dict(weight_init=0.0), dict(weight_final=float("nan")), dict(num_iterations=0),
                dict(min_coverage=1.5), dict(min_coverage=float("nan")), dict(depth_scale=0.0), dict(depth_scale=float("inf"))):
        with pytest.raises(ValueError):
            depth.DepthConfig(**bad).check()
    cfg = depth.DepthConfig(weight_init=1.0, weight_final=0.01, num_iterations=100)
    cfg.check()
    assert (cfg.space, cfg.norm, cfg.min_coverage, cfg.depth_scale) == ("inverse", "l1", 0.5, None)
    assert cfg.weight_at(0) == 1.0 and abs(cfg.weight_at(50) - 0.1) < 1e-12 and abs(cfg.weight_at(1000) - 0.01) < 1e-12
    assert depth.DepthConfig(weight_init=0.3).weight_at(7) == 0.3


def test_trainer_takes_the_switch_and_keeps_its_config():
    import dataclasses
    import inspect
    from taichi_3d_gaussian_splatting_amd.GaussianPointTrainer import GaussianPointCloudTrainer
    params = inspect.signature(GaussianPointCloudTrainer.__init__).parameters
    assert params["depth"].default == "none" and params["depth_config"].default is None
    assert not any("depth" in f.name for f in dataclasses.fields(GaussianPointCloudTrainer.TrainConfig))
    config = GaussianPointCloudTrainer.TrainConfig()
    from taichi_3d_gaussian_splatting_amd.depth import DepthConfig
    with pytest.raises(ValueError, match="depth"):
        GaussianPointCloudTrainer(config, depth="lidar")
    with pytest.raises(ValueError, match="depth_config"):
        GaussianPointCloudTrainer(config, depth_config=DepthConfig())
    with pytest.raises(ValueError, match="space"):
        GaussianPointCloudTrainer(config, depth="relative", depth_config=DepthConfig(space="depth"))
    with pytest.raises(ValueError, match="targets_on_device"):
        GaussianPointCloudTrainer(dataclasses.replace(config, targets_on_device=False), depth="metric")
    rgb_only = GaussianPointCloudTrainer.TrainConfig()
    rgb_only.rasterisation_config.rgb_only = True
    with pytest.raises(ValueError, match="rgb_only"):
        GaussianPointCloudTrainer(rgb_only, depth="metric")


def _dataset(tmp_path, depth_paths=None, depth_scales=None, size=(48, 40)):
    """a dataset JSON of two 48x40 pictures (width x height), with the given depth columns"""
    import PIL.Image
    records = []
    for i in range(2):
        image_path = str(tmp_path / f"image_{i}.png")
        PIL.Image.fromarray(np.full((size[1], size[0], 3), 40 * i, np.uint8)).save(image_path)
        record = dict(image_path=image_path, T_pointcloud_camera=np.eye(4).tolist(), camera_intrinsics=[[50.0, 0, 24], [0, 50.0, 20], [0, 0, 1]],
                      camera_height=size[1], camera_width=size[0], camera_id=0)
        if depth_paths is not None:
            record["depth_path"] = depth_paths[i]
        if depth_scales is not None:
            record["depth_scale"] = depth_scales[i]
        records.append(record)
    path = str(tmp_path / "dataset.json")
    with open(path, "w") as fh:
        json.dump(records, fh)
    return path


def test_load_depth_reads_16_bit_pngs_and_npy_files(tmp_path):
    import PIL.Image
    from taichi_3d_gaussian_splatting_amd.ImagePoseDataset import ImagePoseDataset
    rng = np.random.default_rng(0)
    png = rng.integers(0, 65536, (40, 48)).astype(np.uint16)
    png[0, 0], png[1, 1] = 0, 65535
    PIL.Image.fromarray(png).save(str(tmp_path / "d0.png"))
    npy = rng.uniform(0.5, 9.0, (40, 48)).astype(np.float32)
    npy[3, 3] = np.nan
    np.save(str(tmp_path / "d1.npy"), npy)
    with PIL.Image.open(str(tmp_path / "d0.png")) as pil:
        assert pil.mode == "I;16"
    ds = ImagePoseDataset(_dataset(tmp_path, [str(tmp_path / "d0.png"), str(tmp_path / "d1.npy")], [0.002, None]))
    d0, s0 = ds.load_depth(0)
    assert d0.dtype == np.uint16 and np.array_equal(d0, png) and s0 == 0.002
    d1, s1 = ds.load_depth(1)
    assert d1.dtype == np.float32 and np.array_equal(d1, npy, equal_nan=True) and s1 is None
    # no column, an empty entry
    assert ImagePoseDataset(_dataset(tmp_path)).load_depth(0) is None
    ds = ImagePoseDataset(_dataset(tmp_path, [str(tmp_path / "d0.png"), ""]))
    assert ds.load_depth(1) is None and ds.load_depth(0)[1] is None
    assert ds.load_mask(0) is None                                  # the mask column is as it was


def test_load_depth_refuses_other_sizes_formats_and_large_pictures(tmp_path):
    import PIL.Image
    from taichi_3d_gaussian_splatting_amd.ImagePoseDataset import ImagePoseDataset
    PIL.Image.fromarray(np.ones((20, 24), np.uint16)).save(str(tmp_path / "small.png"))
    np.save(str(tmp_path / "small.npy"), np.ones((40, 47), np.float32))
    PIL.Image.fromarray(np.ones((40, 48), np.uint8)).save(str(tmp_path / "eight.png"))
    np.save(str(tmp_path / "int.npy"), np.ones((40, 48), np.int32))
    for name, match in (("small.png", "24x20"), ("small.npy", "47x40"), ("eight.png", "16-bit"), ("int.npy", "float")):
        ds = ImagePoseDataset(_dataset(tmp_path, [str(tmp_path / name)] * 2))
        with pytest.raises(ValueError, match=match):
            ds.load_depth(0)
    PIL.Image.fromarray(np.ones((16, 1616), np.uint16)).save(str(tmp_path / "wide.png"))
    ds = ImagePoseDataset(_dataset(tmp_path, [str(tmp_path / "wide.png")] * 2, size=(1616, 16)))
    with pytest.raises(ValueError, match="autoscale"):
        ds.load_depth(0)


def test_product_sources_do_not_mention_the_checker():
    for path in (os.path.join(PKG, "depth.py"), os.path.join(PKG, "csrc", "k_depth.hip"), HEADER):
        assert "oracle" not in open(path).read().lower(), path
