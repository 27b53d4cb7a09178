"""CPU: the gs_backward_extra struct of include/gs_rasterizer.h against its ctypes mirror (gcc sizeof / offsetof probe), and the
binding of gs_backward_ex."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gs_rasterizer.h")


def test_backward_extra_layout_matches_the_header(tmp_path):
    from taichi_3d_gaussian_splatting_amd import _native
    cls = _native.GsBackwardExtra
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){',
             'printf("size %zu\\n", sizeof(gs_backward_extra));']
    for fname, _ in cls._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(gs_backward_extra, {fname}));')
    lines.append("return 0; }")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["size"]) == C.sizeof(cls)
    assert [f for f, _ in cls._fields_] == ["grad_rasterized_depth", "rasterized_depth", "grad_pixel_accumulated_alpha"]
    for fname, _ in cls._fields_:
        assert int(got[fname]) == getattr(cls, fname).offset, fname


def test_backward_ex_is_bound():
    from taichi_3d_gaussian_splatting_amd import _native
    L = _native.lib()
    assert "gs_backward_ex" in _native.SYMBOLS and hasattr(L, "gs_backward_ex")
    assert len(L.gs_backward_ex.argtypes) == 12
    assert L.gs_backward_ex.argtypes[6] is C.POINTER(_native.GsBackwardExtra)


def test_config_switch_defaults_to_the_reference_behaviour():
    from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast
    cfg = Rast.GaussianPointCloudRasterisationConfig()
    assert cfg.differentiable_depth is False
    assert "differentiable_depth" not in Rast.GaussianPointCloudRasterisationConfig.__dataclass_fields__   # a class attribute
