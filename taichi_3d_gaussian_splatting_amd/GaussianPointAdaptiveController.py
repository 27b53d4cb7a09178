"""GaussianPointAdaptiveController -- drop-in for the reference's adaptive density controller
(taichi_3d_gaussian_splatting/GaussianPointAdaptiveController.py, CTRL below) backed by libgsrast.

Same class, nested dataclass names and fields, method names and iteration schedule as the reference.  The decisions
and edits of _find_densify_points / _add_densify_points (CTRL:170-353, two Taichi kernels and ~40 torch launches with
host syncs in the reference) are two library calls, gs_density_select and gs_density_apply, that never wait for the
host; update()'s six accumulations (CTRL:133-141) are gs_controller_accumulate or, when the rasteriser was given the
controller's accumulators, the backward kernel itself.  There is no Taichi and no fallback path; the library calls go
through _native.call().

Deviation (DESIGN.md "Numerics"): the split samples of GaussianPoint3D.sample() draw from Philox4x32-10 keyed by
`seed`, not from Taichi's ti.random(): the same distribution, a different (reproducible) stream.
Not for data-parallel training as is: the single-frame and floater criteria come from one rank's view, so replicas
would take different decisions (ControllerAccumulators.all_reduce covers only the statistics).
"""
from dataclasses import dataclass

import torch

from . import _native
from ._host import _ConfigBase, _require
from ._native import ptr as _ptr
from .GaussianPointCloudRasterisation import GaussianPointCloudRasterisation
from .controller_stats import ControllerAccumulators


class GaussianPointAdaptiveController:
    """
    For simplicity, the size of the point cloud is fixed during training; point_invalid_mask marks the free rows.
    Densified points are written into free rows (point_invalid_mask == 1), removed points only get the mask set.
    """
    @dataclass
    class GaussianPointAdaptiveControllerConfig(_ConfigBase):         # CTRL:54-84, same fields and defaults
        num_iterations_warm_up: int = 500
        num_iterations_densify: int = 100
        transparent_alpha_threshold: float = -0.5
        densification_view_space_position_gradients_threshold: float = 6e-6
        densification_view_avg_space_position_gradients_threshold: float = 1e3
        densification_multi_frame_view_space_position_gradients_threshold: float = 1e3
        densification_multi_frame_view_pixel_avg_space_position_gradients_threshold: float = 1e3
        densification_multi_frame_position_gradients_threshold: float = 1e3
        gaussian_split_factor_phi: float = 1.6
        num_iterations_reset_alpha: int = 3000
        reset_alpha_value: float = 0.1
        floater_num_pixels_threshold: int = 10000               # unused by the reference too (CTRL:194, commented out)
        floater_near_camrea_num_pixels_threshold: int = 10000
        floater_depth_threshold: float = 100
        iteration_start_remove_floater: int = 2000
        plot_densify_interval: int = 200                        # kept for YAML compatibility; there are no plots here
        under_reconstructed_num_pixels_threshold: int = 512
        under_reconstructed_move_factor: float = 100.0
        enable_ellipsoid_offset: bool = False
        enable_sample_from_point: bool = True

    @dataclass
    class GaussianPointAdaptiveControllerMaintainedParameters:    # CTRL:86-93
        pointcloud: torch.Tensor            # (N,3) f32
        pointcloud_features: torch.Tensor   # (N,56) f32
        point_invalid_mask: torch.Tensor    # (N,) i8, 1 = free row
        point_object_id: torch.Tensor       # (N,) i32

    def __init__(self, config: "GaussianPointAdaptiveController.GaussianPointAdaptiveControllerConfig",
                 maintained_parameters: "GaussianPointAdaptiveController.GaussianPointAdaptiveControllerMaintainedParameters",
                 seed: int = 0, rasteriser_accumulates: bool = False, verbose: bool = False):
        """Extensions over the reference signature (CTRL:106-108):
        seed                    key of the split samples' random stream (Philox4x32-10).
        rasteriser_accumulates  False: update() adds the hook payload to `self.accumulators` (the reference's wiring,
                                backward_valid_point_hook=controller.update).  True: the rasteriser was constructed with
                                controller_accumulators=controller.accumulators and adds them in its backward kernel;
                                update() then only keeps the schedule and selects.
        verbose                 print what the reference prints at each densification (reads the counts: syncs)."""
        mp = maintained_parameters
        dev = mp.pointcloud.device
        n = mp.pointcloud.shape[0]
        _require(mp.pointcloud, "pointcloud", torch.float32, (3,))
        _require(mp.pointcloud_features, "pointcloud_features", torch.float32, (56,), dev)
        _require(mp.point_invalid_mask, "point_invalid_mask", torch.int8, (), dev)
        _require(mp.point_object_id, "point_object_id", torch.int32, (), dev)
        if not (mp.pointcloud_features.shape[0] == mp.point_invalid_mask.shape[0] == mp.point_object_id.shape[0] == n):
            raise ValueError("the maintained parameters disagree on N")
        self.iteration_counter = -1
        self.config = config
        self.maintained_parameters = mp
        self.input_data = None
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.rasteriser_accumulates = bool(rasteriser_accumulates)
        self.verbose = bool(verbose)
        self.has_plot = False                                   # the reference's matplotlib plot: never drawn here
        self.accumulators = ControllerAccumulators.zeros(n, dev)
        self.refinement_calls = 0                               # densifications applied so far (the sample counter)
        self._selected = False
        self._device = dev
        self._context = _native.Context(_native.device_index(dev))
        # the plan: caller-owned device arrays, allocated once for N rows
        z = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype, device=dev)
        self._flags = z(n, dtype=torch.int8)
        self._densify_ids = z(n, dtype=torch.int32)
        self._densify_pos = z(n, 3, dtype=torch.float32)
        self._densify_grad = z(n, 3, dtype=torch.float32)
        self._densify_factor = z(n, dtype=torch.float32)
        self._fill_ids = z(n, dtype=torch.int32)
        self._scratch = z(int(_native.lib().gs_density_scratch_bytes(n)), dtype=torch.uint8)
        self._counts = z(len(_native.DENSITY_COUNTS), dtype=torch.int32)
        self._plan = _native.GsDensityPlan(
            flags=_ptr(self._flags), densify_point_id=_ptr(self._densify_ids),
            densify_point_position_before_optimization=_ptr(self._densify_pos), densify_point_grad_position=_ptr(self._densify_grad),
            densify_size_reduction_factor=_ptr(self._densify_factor), fill_point_id=_ptr(self._fill_ids), scratch=_ptr(self._scratch),
            counts=_ptr(self._counts), n_points=n)

    # the reference keeps the six statistics as attributes of the controller (CTRL:114-127)
    def __getattr__(self, name):
        if name.startswith("accumulated_") and "accumulators" in self.__dict__:
            return getattr(self.__dict__["accumulators"], name)
        raise AttributeError(name)

    # ------------------------------------------------------------------ library plumbing
    def _n(self) -> int:
        return self.maintained_parameters.pointcloud.shape[0]

    def _call(self, name, *args):
        _native.call(name, self._device, self._context.handle, *args)

    def _c_scene(self):
        mp = self.maintained_parameters
        return _native.GsScene.of(mp.pointcloud, mp.pointcloud_features, mp.point_invalid_mask, mp.point_object_id)

    def _check_scene(self):
        mp = self.maintained_parameters
        for t in (mp.pointcloud, mp.pointcloud_features, mp.point_invalid_mask, mp.point_object_id):
            if t.shape[0] != self._n() or not t.is_contiguous() or t.device != self._device:
                raise ValueError("the maintained parameters changed shape, layout or device since the controller was built")

    # ------------------------------------------------------------------ the reference's interface
    def update(self, input_data: GaussianPointCloudRasterisation.BackwardValidPointHookInput):   # CTRL:130-145
        self.iteration_counter += 1
        with torch.no_grad():
            ids = input_data.point_id_in_camera_list
            m = ids.shape[0]
            dev = self._device
            if not self.rasteriser_accumulates:
                _require(ids, "point_id_in_camera_list", torch.int32, (), dev)
                _require(input_data.num_affected_pixels, "num_affected_pixels", torch.int32, (), dev)
                _require(input_data.magnitude_grad_viewspace, "magnitude_grad_viewspace", torch.float32, (), dev)
                _require(input_data.grad_point_in_camera, "grad_point_in_camera", torch.float32, (3,), dev)
                self._call("gs_controller_accumulate", _ptr(ids), _ptr(input_data.num_affected_pixels),
                           _ptr(input_data.magnitude_grad_viewspace), _ptr(input_data.grad_point_in_camera), m, self._n(),
                           _native.GsControllerAccumulators.of(self.accumulators))
            if self.iteration_counter < self.config.num_iterations_warm_up:
                pass
            elif self.iteration_counter % self.config.num_iterations_densify == 0:
                self._find_densify_points(input_data)
                self.input_data = input_data

    def refinement(self):                                                                         # CTRL:147-168
        with torch.no_grad():
            if self.iteration_counter < self.config.num_iterations_warm_up:
                return
            if self.iteration_counter % self.config.num_iterations_densify == 0:
                self._add_densify_points()
                self.accumulators.reset()
            if self.iteration_counter % self.config.num_iterations_reset_alpha == 0:
                self.reset_alpha()
            self.input_data = None

    def _find_densify_points(self, input_data: GaussianPointCloudRasterisation.BackwardValidPointHookInput):
        """CTRL:170-265 as one library call, inside the backward, before the optimiser step: the masks, the densify ids
        and the snapshots of their positions and position gradients stay in the plan on the device."""
        self._check_scene()
        dev = self._device
        ids = input_data.point_id_in_camera_list
        for t, name, dtype in [(ids, "point_id_in_camera_list", torch.int32), (input_data.num_affected_pixels, "num_affected_pixels", torch.int32),
                               (input_data.point_depth, "point_depth", torch.float32),
                               (input_data.magnitude_grad_viewspace, "magnitude_grad_viewspace", torch.float32)]:
            _require(t, name, dtype, (), dev)
            if t.shape[0] != ids.shape[0]:
                raise ValueError("the hook arrays disagree on M")
        remove_floaters = 1 if self.iteration_counter > self.config.iteration_start_remove_floater else 0   # CTRL:191
        self._call("gs_density_select", self._c_scene(), _native.GsControllerAccumulators.of(self.accumulators), _ptr(ids),
                   _ptr(input_data.num_affected_pixels), _ptr(input_data.point_depth), _ptr(input_data.magnitude_grad_viewspace),
                   ids.shape[0], remove_floaters, _native.GsDensityConfig.of(self.config), self._plan)
        self._selected = True
        if self.verbose:
            c = self.last_refinement_counts()
            print(f"num_to_densify: {c['single_frame']}, num_to_densify_by_viewspace: {c['single_frame_viewspace']}, "
                  f"num_to_densify_by_viewspace_avg: {c['single_frame'] - c['single_frame_viewspace']}")
            print(f"num_merged_densify_with_multi_frame: {c['densify']}")

    def _add_densify_points(self):
        """CTRL:290-353 as one library call, after the optimiser step."""
        assert self._selected, "refinement() at a densify iteration without the backward hook having run (CTRL:291)"
        self._check_scene()
        self._call("gs_density_apply", self._c_scene(), _native.GsDensityConfig.of(self.config), self._plan, self.seed,
                   self.refinement_calls & 0xFFFFFFFF)
        self.refinement_calls += 1
        self._selected = False
        if self.verbose:
            c = self.last_refinement_counts()
            print(f"num_over_reconstructed: {c['over']}, num_under_reconstructed: {c['under']}")
            print(f"total valid points: {c['valid_before']} -> {c['valid_after']}, num_densify_points: {c['densify']}, "
                  f"num_fillable_densify_points: {c['fillable']}")
            print(f"num_transparent_points: {c['transparent']}, num_floaters_points: {c['floaters']}")

    def reset_alpha(self):                                                                        # CTRL:355-358
        with torch.no_grad():
            self.maintained_parameters.pointcloud_features[:, 7].clamp_(max=self.config.reset_alpha_value)

    # ------------------------------------------------------------------ extensions
    def last_refinement_counts(self) -> dict:
        """The counts of the last select / apply (include/gs_rasterizer.h gs_density_count).  The only call of this
        class that waits for the device."""
        return dict(zip(_native.DENSITY_COUNTS, self._counts.tolist()))

    def densify_plan(self) -> dict:
        """The device arrays of the last select / apply, views of the plan (for inspection; valid until the next call)."""
        c = self.last_refinement_counts()
        nd, nf = c["densify"], c["fillable"]
        return dict(flags=self._flags, densify_point_id=self._densify_ids[:nd],
                    densify_point_position_before_optimization=self._densify_pos[:nd],
                    densify_point_grad_position=self._densify_grad[:nd], densify_size_reduction_factor=self._densify_factor[:nd],
                    fill_point_id=self._fill_ids[:nf], counts=c)
