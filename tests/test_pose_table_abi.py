"""CPU: the C ABI of the pose corrections (include/gs_pose_table.h) and its binding (pose_table.py)."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gs_pose_table.h")
PKG = os.path.join(ROOT, "taichi_3d_gaussian_splatting_amd")
NAMES = ["gs_pose_compose", "gs_pose_compose_backward"]
INVALID = -1                                                      # GS_ERR_INVALID_ARGUMENT


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w ]*?[\w*])\s+(gs_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        types = [re.sub(r"\bconst\b|\s", "", re.match(r"(.*?)(\w+)$", p.strip()).group(1)) for p in params.split(",")]
        protos[name] = (ret.strip(), types)
    return protos


def _define(name):
    return float(re.search(r"#define\s+%s\s+([0-9.e+-]+)" % name, open(HEADER).read()).group(1))


def test_header_is_plain_c99_and_declares_the_functions(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(f'#include "{HEADER}"\n'
                   'int main(void) {\n'
                   '  int (*f)(gs_ctx*, const float*, const float*, const float*, int32_t, int32_t, float*, float*, gs_stream) = gs_pose_compose;\n'
                   '  int (*g)(gs_ctx*, const float*, const float*, const float*, const float*, int32_t, int32_t, float, float*, gs_stream) =\n'
                   '      gs_pose_compose_backward;\n'
                   '  (void)f; (void)g;\n'
                   '  return GS_POSE_DELTA_FLOATS == 6 && GS_POSE_THREADS == 256 && GS_POSE_SERIES_S == 1e-8 ? 0 : 1; }\n')
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
    assert "gs_pose_compose" not in open(os.path.join(ROOT, "include", "gs_rasterizer.h")).read()
    makefile = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "k_posetable.hip" in makefile and "gs_pose_table.h" in makefile


def test_argtypes_match_the_prototypes():
    from taichi_3d_gaussian_splatting_amd import _native, pose_table
    pose_table._bind()
    L = _native.lib()
    kinds = {"gs_ctx*": C.c_void_p, "float*": C.c_void_p, "gs_stream": C.c_void_p, "int32_t": C.c_int32, "float": C.c_float}
    protos = _prototypes()
    assert sorted(pose_table.ARGTYPES) == NAMES
    for name in NAMES:
        ret, params = protos[name]
        assert ret == "int" and params[-1] == "gs_stream"          # _native.call() appends the stream
        assert name not in _native._STREAMLESS
        fn = getattr(L, name)
        assert fn.restype is C.c_int
        assert list(fn.argtypes) == [kinds[p] for p in params] == pose_table.ARGTYPES[name], name


def test_macros_agree_between_the_header_python_and_the_reference():
    from taichi_3d_gaussian_splatting_amd import pose_table
    import pose_table_ref
    assert _define("GS_POSE_DELTA_FLOATS") == pose_table.DELTA_FLOATS == pose_table_ref.DELTA_FLOATS == 6
    assert _define("GS_POSE_THREADS") == pose_table.THREADS == pose_table_ref.THREADS == 256
    assert _define("GS_POSE_SERIES_S") == pose_table.SERIES_S == pose_table_ref.SERIES_S == 1e-8
    assert _define("GS_POSE_MAX_VIEWS") == pose_table.MAX_VIEWS == pose_table_ref.MAX_VIEWS == 2 ** 24
    assert _define("GS_POSE_MAX_OBJECTS") == pose_table.MAX_OBJECTS == pose_table_ref.MAX_OBJECTS == 64


def test_bad_arguments_are_refused_without_a_gpu():
    """argument checks come before anything that needs a device"""
    from taichi_3d_gaussian_splatting_amd import _native, pose_table
    pose_table._bind()
    L = _native.lib()
    compose, backward, err = L.gs_pose_compose, L.gs_pose_compose_backward, L.gs_last_error
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert compose(None, p, p, p, 1, 1, p, p, None) == INVALID and b"ctx is NULL" in err()
    assert backward(None, p, p, p, p, 1, 1, 0.0, p, None) == INVALID and b"ctx is NULL" in err()
    ctx = C.c_void_p(8)       # a context handle that is never dereferenced: everything below is refused before it is looked at
    for V, K, what in ((-1, 1, b"V must"), (2 ** 24 + 1, 1, b"V must"), (1, -1, b"K must"), (1, 65, b"K must")):
        assert compose(ctx, p, p, p, V, K, p, p, None) == INVALID and what in err()
        assert backward(ctx, p, p, p, p, V, K, 0.0, p, None) == INVALID and what in err()
    for i in range(5):
        args = [p] * 5
        args[i] = None
        assert compose(ctx, args[0], args[1], args[2], 1, 1, args[3], args[4], None) == INVALID and b"NULL array" in err()
        assert backward(ctx, args[0], args[1], args[2], args[3], 1, 1, 0.0, args[4], None) == INVALID and b"NULL array" in err()
    for reg in (float("nan"), float("inf")):
        assert backward(ctx, p, p, p, p, 1, 1, reg, p, None) == INVALID and b"reg must be finite" in err()
    # nothing to do is not an error, and needs no array
    assert compose(ctx, None, None, None, 0, 1, None, None, None) == 0 and compose(ctx, None, None, None, 1, 0, None, None, None) == 0
    assert backward(ctx, None, None, None, None, 0, 3, 0.0, None, None) == 0


def test_cpu_tensors_wrong_dtypes_and_shapes_are_refused_in_python():
    from taichi_3d_gaussian_splatting_amd import pose_table
    q, t, d = torch.zeros(2, 3, 4), torch.zeros(2, 3, 3), torch.zeros(2, 6)
    for call in (lambda: pose_table.compose(q, t, d), lambda: pose_table.compose_forward(q, t, d), lambda: pose_table.compose(q[0], t[0], d[0]),
                 lambda: pose_table.compose_backward(q, d, q, t)):
        with pytest.raises(ValueError, match="GPU"):
            call()
    with pytest.raises(ValueError, match="GPU"):
        pose_table.PoseTable(3, "cpu")
    # what is wrong with a tensor is found before its device is looked at
    with pytest.raises(TypeError, match="float32"):
        pose_table.compose(q.double(), t, d)
    with pytest.raises(TypeError, match="tensor"):
        pose_table.compose_forward(q.numpy(), t, d)
    for bad in (torch.zeros(2, 3, 3), torch.zeros(2, 3, 4, 1)):
        with pytest.raises(ValueError, match=r"\(V,K,4\)"):
            pose_table.compose_forward(bad, t, d)

    # the checks behind the device test, against poses that are on no CPU
    fq = torch.zeros(2, 3, 4, device="meta")
    for bad, exc in ((torch.zeros(3, 6, device="meta"), ValueError), (torch.zeros(2, 6, dtype=torch.float16, device="meta"), TypeError),
                     (torch.zeros(2, 12, device="meta")[:, ::2], ValueError), (torch.zeros(2, 6), ValueError), (None, TypeError)):
        with pytest.raises(exc, match="delta"):
            pose_table.check_delta(bad, fq)
    for bad in (dict(lr=0.0), dict(lr_final=float("nan")), dict(num_iterations=0), dict(start_iteration=-1), dict(reg=-1.0),
                dict(reg=float("inf")), dict(betas=(1.0, 0.999)), dict(eps=0.0)):
        with pytest.raises(ValueError):
            pose_table.PoseRefinementConfig(**bad).check()
    config = pose_table.PoseRefinementConfig(num_iterations=100, start_iteration=20)
    assert config.lr_at(0) == config.lr_at(20) and abs(config.lr_at(20) - config.lr) < 1e-18 and abs(config.lr_at(100) - config.lr_final) < 1e-18
    assert config.lr_final < config.lr_at(60) < config.lr


def test_trainer_takes_the_switch_and_keeps_its_config():
    import dataclasses
    import inspect
    from taichi_3d_gaussian_splatting_amd.GaussianPointTrainer import GaussianPointCloudTrainer
    params = inspect.signature(GaussianPointCloudTrainer.__init__).parameters
    assert params["pose_refinement"].default is None and params["validation_pose_steps"].default == 0
    assert not any("pose" in f.name for f in dataclasses.fields(GaussianPointCloudTrainer.TrainConfig))


def test_product_sources_do_not_mention_the_checker():
    for path in (os.path.join(PKG, "pose_table.py"), os.path.join(PKG, "csrc", "k_posetable.hip"), HEADER):
        assert "oracle" not in open(path).read().lower(), path
