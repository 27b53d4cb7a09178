"""CPU: the binding of gs_backward_ex and the config switch of the depth gradient (the layout of gs_backward_extra is probed
with every other struct in test_abi.py)."""
import ctypes as C


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
