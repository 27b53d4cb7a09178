"""CPU: the pieces of the on-device adaptive density controller that need no GPU -- the Philox4x32-10 restatement
the device stream is checked against and the config defaults (the ABI structs are probed in test_abi.py)."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from density_ref import philox4x32_10_numpy, philox4x32_10_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Random123's known-answer vectors for philox4x32 with 10 rounds (kat_vectors)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert tuple(int(v) for v in philox4x32_10_numpy(np.array(ctr, np.uint32), key)) == want
    assert tuple(philox4x32_10_torch(torch.tensor(ctr, dtype=torch.int64), key).tolist()) == want


def test_philox_torch_and_numpy_agree_on_many_counters():
    rng = np.random.default_rng(3)
    ctr = rng.integers(0, 2 ** 32, (1000, 4), dtype=np.uint64).astype(np.uint32)
    key = (0x12345678, 0x9abcdef0)
    a = philox4x32_10_numpy(ctr, key)
    b = philox4x32_10_torch(torch.tensor(ctr.astype(np.int64)), key).numpy().astype(np.uint32)
    assert np.array_equal(a, b)


def test_density_symbols_are_bound_and_not_timed_kernels():
    from taichi_3d_gaussian_splatting_amd import _native
    L = _native.lib()
    for s in ["gs_density_scratch_bytes", "gs_density_select", "gs_density_apply", "gs_controller_accumulate"]:
        assert s in _native.SYMBOLS and hasattr(L, s)
    assert "density" not in L.gs_kernel_names().decode()          # the list is one forward+backward's kernels
    assert L.gs_density_scratch_bytes(0) > 0
    assert L.gs_density_scratch_bytes(10 ** 6) >= 5 * 4 * (10 ** 6 // 256)
    assert L.gs_density_scratch_bytes(-1) == 0


def test_config_defaults_equal_the_reference():
    """GaussianPointAdaptiveControllerConfig, CTRL:54-84: same fields, same order, same defaults."""
    from taichi_3d_gaussian_splatting_amd import GaussianPointAdaptiveController
    cfg = GaussianPointAdaptiveController.GaussianPointAdaptiveControllerConfig()
    want = [("num_iterations_warm_up", 500), ("num_iterations_densify", 100), ("transparent_alpha_threshold", -0.5),
            ("densification_view_space_position_gradients_threshold", 6e-6),
            ("densification_view_avg_space_position_gradients_threshold", 1e3),
            ("densification_multi_frame_view_space_position_gradients_threshold", 1e3),
            ("densification_multi_frame_view_pixel_avg_space_position_gradients_threshold", 1e3),
            ("densification_multi_frame_position_gradients_threshold", 1e3), ("gaussian_split_factor_phi", 1.6),
            ("num_iterations_reset_alpha", 3000), ("reset_alpha_value", 0.1), ("floater_num_pixels_threshold", 10000),
            ("floater_near_camrea_num_pixels_threshold", 10000), ("floater_depth_threshold", 100),
            ("iteration_start_remove_floater", 2000), ("plot_densify_interval", 200),
            ("under_reconstructed_num_pixels_threshold", 512), ("under_reconstructed_move_factor", 100.0),
            ("enable_ellipsoid_offset", False), ("enable_sample_from_point", True)]
    got = [(f.name, getattr(cfg, f.name)) for f in dataclasses.fields(cfg)]
    assert got == want
    mp = GaussianPointAdaptiveController.GaussianPointAdaptiveControllerMaintainedParameters
    assert [f.name for f in dataclasses.fields(mp)] == ["pointcloud", "pointcloud_features", "point_invalid_mask", "point_object_id"]


def test_device_config_rounds_like_torch():
    """What the kernels compare against: f32 thresholds, log(phi) rounded once on the host, integer pixel thresholds."""
    from taichi_3d_gaussian_splatting_amd import GaussianPointAdaptiveController as Ctl, _native
    cfg = Ctl.GaussianPointAdaptiveControllerConfig(under_reconstructed_num_pixels_threshold=511.5)
    c = _native.GsDensityConfig.of(cfg)
    assert c.log_gaussian_split_factor_phi == float(np.float32(np.log(1.6)))
    assert c.densification_view_space_position_gradients_threshold == float(np.float32(6e-6))
    assert c.under_reconstructed_num_pixels_threshold == 511          # int > 511.5  <=>  int > 511
    assert c.floater_near_camrea_num_pixels_threshold == 10000 and c.enable_sample_from_point == 1 and c.enable_ellipsoid_offset == 0


def test_package_imports_no_taichi():
    out = subprocess.check_output([sys.executable, "-c", "import sys, taichi_3d_gaussian_splatting_amd as t; t.GaussianPointAdaptiveController; "
                                   "print(any(m.split('.')[0] in ('taichi', 'matplotlib') for m in sys.modules))"], cwd=ROOT)
    assert out.decode().strip() == "False"
