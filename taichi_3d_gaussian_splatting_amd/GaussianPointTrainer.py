"""GaussianPointCloudTrainer -- the reference's training loop (taichi_3d_gaussian_splatting/GaussianPointTrainer.py, TRAIN
below) over this package's pieces: GaussianPointCloudScene, the rasteriser with the adaptive controller's update as its
backward hook, the fused LossFunction and FusedAdam.  Same class and config names, fields, defaults, schedules, log tags and
checkpoint files, so the reference's YAMLs and dataset JSONs work unchanged.

What differs from the reference
  - Targets come from targets.TargetStore by default (targets_on_device=True): images resident on the device as uint8, one
    kernel per step.  targets_on_device=False is the reference's path, kept for comparison: ImagePoseDataset through a
    DataLoader (num_workers=0) and the antialiased resize on the CPU.
  - The view order is a seeded torch.randperm per epoch (trainer.view_order), not a shuffling DataLoader.
  - The clamp of the predicted image runs inside the loss kernels (clamp_predicted=True), and SSIM for the logged metrics is
    1 - the loss's third term instead of pytorch_msssim.
  - GaussianPointCloudTrainer(config, pixel_weights="alpha" | "file") trains with a weight per pixel (masked training): the
    store hands the weight out with the target, in the same launch, and the fused loss takes it (LossFunction's pixel_weight).
    "none", the default, is the loop as it was.  These two settings are constructor arguments like device and writer:
    TrainConfig keeps the reference's fields and the three extensions it has.
  - GaussianPointCloudTrainer(config, density="mcmc", mcmc_config=MCMCConfig(cap_max=...)) trains with a fixed budget of
    Gaussians (mcmc.py): no adaptive controller and no backward hook; the strategy's two calls bracket the optimiser steps.
    "adaptive", the default, is the loop as it was.
  - GaussianPointCloudTrainer(config, appearance="affine", appearance_config=AppearanceConfig(...)) trains a 3x4 affine colour
    transform per training image with the scene (appearance.py): exposure compensation for captures whose exposure and white
    balance differ between views.  The transform is applied to the rendered image in front of the loss; validation views have
    none and are rendered uncorrected, and additionally measured after the best affine fit to their ground truth (val/psnr_cc,
    val/ssim_cc, val/loss_cc).  "none", the default, is the loop as it was.
  - GaussianPointCloudTrainer(config, bilateral_grid=BilateralGridConfig(...)) trains a bilateral grid per training image with
    the scene (bilateral.py): a lattice of 3x4 colour transforms over the image plane and the rendered luminance, sliced at
    every pixel in front of the loss -- it contains the affine transform and also absorbs what varies across the picture
    (vignetting, local tone mapping).  After the backward the total variation of the step's own grid, times tv_weight, is
    added to that grid's gradient (gsplat regularises every view's grid every step; here a step's cost does not grow with the
    number of views), then that grid alone takes an Adam step.  Validation is as with appearance="affine".  None, the
    default, is the loop as it was.
  - GaussianPointCloudTrainer(config, depth="metric" | "relative", depth_config=DepthConfig(...)) adds a depth term to the loss
    (depth.py): the dataset's depth_path maps -- metres for "metric", a monocular network's relative inverse depth for
    "relative", aligned per view by a closed-form scale and shift -- resident on the device, one launch per step for the
    target and its validity weight, and the fused masked depth loss on the rasteriser's depth output.  "none", the default, is
    the loop as it was.
  - GaussianPointCloudTrainer(config, geometry=GeometryConfig(smooth_weight=..., normal_weight=...)) adds geometry regularisers
    on the rendered depth (geometry.py): an edge-aware smoothness with the colour target as its guide -- it needs no extra data
    -- and a cosine loss of the depth-derived normal against the dataset's normal_path priors, resident on the device.  None,
    the default, is the loop as it was.
  - GaussianPointCloudTrainer(config, background="colour" | "random" | "sky", background_config=BackgroundConfig(...),
    composite_targets=False) puts a background behind the splats (background.py): the step's forward also returns the
    accumulated alpha, and the rendered image is composited over a solid colour, a random colour drawn per step, or a learnable
    spherical-harmonics sky, before any appearance transform or bilateral grid (the camera's processing acts on the whole
    picture).  composite_targets=True composites the RGBA training pictures over the step's colour too, so the transparent
    pixels tell the scene to be empty; "random" needs it.  "sky" takes its Adam step beside the scene's.  Validation composites
    with the model's stored background (config.colour for "random").  "none", the default, is the loop as it was.
  - GaussianPointCloudTrainer(config, filter3d=Filter3DConfig(...)) trains under the 3D smoothing filter of Mip-Splatting
    (filter3d.py): every Gaussian carries the largest sampling rate any training view had of it, and the rasteriser is given
    the scene's features under the matching low-pass, at the step's downsample factor in training and at factor 1 in
    validation.  The rates are recomputed at iteration 0, every filter3d.interval iterations and after every refinement that
    changed rows.  The loss's regulariser, the controller, the fixed-budget strategy and FusedAdam keep reading the raw
    parameters.  filter3d_<iteration>.pt and best_filter3d.pt are written beside the scene files, which stay raw.  None, the
    default, is the loop as it was.
  - GaussianPointCloudTrainer(config, pose_refinement=PoseRefinementConfig(...), validation_pose_steps=0) trains a pose
    correction per training image with the scene (pose_table.py): six floats in the camera's own frame, composed on the right
    of the dataset's pose in front of the rasteriser, trained from the rasteriser's pose gradients and stepped after the two
    scene optimisers, from config.start_iteration on.  self.current_pose and the pose handed to the background are the composed
    values, detached: the sky's gradient to the pose is not taken.  Validation views have no correction and render under the
    dataset's poses; with validation_pose_steps > 0 each is additionally aligned against the frozen scene (refine_pose) and
    measured again (val/psnr_aligned, val/ssim_aligned, val/loss_aligned).  poses_<iteration>.pt and best_poses.pt are written
    beside the scene files.  None, the default, is the loop as it was.
  - TrainConfig.from_yaml_file needs no dataclass_wizard; keys it does not know are listed, not fatal.
  - Logging falls back to a JSON-lines writer when tensorboard is not installed; image grids, figures and histograms are not
    produced, and with them the reference's per-iteration loss.item() (it picks "problematic" images to log): the host waits
    for the device only at the logging intervals.  The FTGMM scene grab (TRAIN:188-189) and the Taichi kernel profiler are
    left out.
"""
import copy
import dataclasses
import json
import os
import typing
from dataclasses import dataclass, field
from typing import List, Optional

import torch

from ._host import _ConfigBase
from .Camera import CameraInfo
from .GaussianPointAdaptiveController import GaussianPointAdaptiveController
from .GaussianPointCloudRasterisation import GaussianPointCloudRasterisation
from .GaussianPointCloudScene import GaussianPointCloudScene
from . import appearance as _appearance
from .appearance import AppearanceConfig, AppearanceTable
from . import background as _background
from .background import BackgroundConfig, BackgroundModel
from . import bilateral as _bilateral
from .bilateral import BilateralGridConfig, BilateralGridTable
from . import depth as _depth
from . import filter3d as _filter3d
from .filter3d import Filter3D, Filter3DConfig
from .depth import DepthConfig
from . import geometry as _geometry
from . import _terms
from .geometry import GeometryConfig
from .ImagePoseDataset import ImagePoseDataset, resize_antialias
from .LossFunction import LossFunction
from .mcmc import MCMCConfig, MCMCStrategy
from .optim import FusedAdam
from . import pose_table as _pose_table
from .pose_table import PoseRefinementConfig, PoseTable
from .targets import TargetStore, downsampled_geometry, downsampled_intrinsics


# ---- the three schedules of TRAIN:143-192 as pure functions of the iteration ----------------------------------------------
def downsample_factor_at(iteration: int, initial_downsample_factor: int, half_downsample_factor_interval: int) -> int:
    """The factor iteration `iteration` trains at: halved at every iteration > 0 that is a multiple of the interval, down to 1
    (TRAIN:144-145)"""
    factor = int(initial_downsample_factor)
    for _ in range(int(iteration) // int(half_downsample_factor_interval)):
        if factor > 1:
            factor //= 2
    return factor


def color_max_sh_band_at(iteration: int, increase_color_max_sh_band_interval) -> int:
    """TRAIN:168 (the interval's default is the float 1000.)"""
    return int(iteration // increase_color_max_sh_band_interval)


def position_learning_rate_at(iteration: int, position_learning_rate: float, decay_rate: float, decay_interval: int) -> float:
    """The position learning rate iteration `iteration` steps with: multiplied by the rate after every earlier iteration that
    is a multiple of the interval -- iteration 0 included, as the reference's scheduler.step() at TRAIN:191-192 has it"""
    lr = float(position_learning_rate)
    for _ in range((int(iteration) + int(decay_interval) - 1) // int(decay_interval)):
        lr *= decay_rate
    return lr


class JsonlSummaryWriter:
    """What the trainer needs of torch.utils.tensorboard.SummaryWriter when tensorboard is not installed: add_scalar appends
    {"tag", "value", "step"} to <log_dir>/metrics.jsonl; images, figures and histograms are accepted and dropped."""

    def __init__(self, log_dir: str):
        os.makedirs(log_dir, exist_ok=True)
        self.log_dir = log_dir
        self.path = os.path.join(log_dir, "metrics.jsonl")
        self._fh = open(self.path, "a")

    def add_scalar(self, tag, scalar_value, global_step=None, walltime=None, **_):
        value = scalar_value.item() if hasattr(scalar_value, "item") else scalar_value
        self._fh.write(json.dumps({"tag": str(tag), "value": float(value), "step": None if global_step is None else int(global_step)}) + "\n")

    def add_image(self, *args, **kwargs):
        pass

    def add_figure(self, *args, **kwargs):
        pass

    def add_histogram(self, *args, **kwargs):
        pass

    def flush(self):
        self._fh.flush()

    def close(self):
        if not self._fh.closed:
            self._fh.close()

    @staticmethod
    def read(path: str) -> List[dict]:
        with open(path) as fh:
            return [json.loads(line) for line in fh if line.strip()]


def make_summary_writer(log_dir: str):
    try:
        from torch.utils.tensorboard import SummaryWriter
    except Exception:
        return JsonlSummaryWriter(log_dir)
    return SummaryWriter(log_dir=log_dir)


def _coerce(value, annotation):
    """A YAML scalar as the field's annotation wants it: PyYAML reads 3e-6 and 1e3 (no dot) as strings, and a float field may
    be written as an integer.  Optional[T] is T unless the value is None; anything else passes as it is."""
    if getattr(annotation, "__origin__", None) is typing.Union:
        inner = [a for a in annotation.__args__ if a is not type(None)]
        annotation = inner[0] if len(inner) == 1 else None
    if value is None or isinstance(value, bool) or annotation not in (int, float, bool):
        return value
    if annotation is bool:
        return {"true": True, "false": False}.get(value.strip().lower(), value) if isinstance(value, str) else value
    if isinstance(value, str):
        number = float(value)
        return int(number) if annotation is int and number == int(number) else number
    return float(value) if annotation is float and isinstance(value, int) else value


def _config_from_dict(cls, data: dict, prefix: str, unknown: List[str]):
    """cls(**data) with keys normalised ('-' -> '_'), nested config dataclasses recursed into and unknown keys collected"""
    fields = {f.name: f for f in dataclasses.fields(cls)}
    hints = {name: f.type for name, f in fields.items() if not isinstance(f.type, str)}
    kwargs = {}
    for key, value in (data or {}).items():
        name = str(key).replace("-", "_")
        if name not in fields:
            unknown.append(prefix + name)
            continue
        default = fields[name].default_factory() if fields[name].default_factory is not dataclasses.MISSING else None
        if dataclasses.is_dataclass(default) and isinstance(value, dict):
            value = _config_from_dict(type(default), value, prefix + name + ".", unknown)
        else:
            value = _coerce(value, hints.get(name))
        kwargs[name] = value
    return cls(**kwargs)


class GaussianPointCloudTrainer:
    @dataclass
    class TrainConfig(_ConfigBase):
        """The reference's fields and defaults (TRAIN:35-63), then three of this package.  enable_taichi_kernel_profiler and
        log_taichi_kernel_profile_interval are accepted and ignored: there is no Taichi here."""
        train_dataset_json_path: str = ""
        val_dataset_json_path: str = ""
        pointcloud_parquet_path: str = ""
        num_iterations: int = 300000
        val_interval: int = 1000
        feature_learning_rate: float = 1e-3
        position_learning_rate: float = 1e-5
        position_learning_rate_decay_rate: float = 0.97
        position_learning_rate_decay_interval: int = 100
        increase_color_max_sh_band_interval: int = 1000.
        log_loss_interval: int = 10
        log_metrics_interval: int = 100
        print_metrics_to_console: bool = False
        log_image_interval: int = 1000
        enable_taichi_kernel_profiler: bool = False
        log_taichi_kernel_profile_interval: int = 1000
        log_validation_image: bool = True
        initial_downsample_factor: int = 4
        half_downsample_factor_interval: int = 250
        summary_writer_log_dir: str = "logs"
        output_model_dir: Optional[str] = None
        rasterisation_config: GaussianPointCloudRasterisation.GaussianPointCloudRasterisationConfig = field(
            default_factory=GaussianPointCloudRasterisation.GaussianPointCloudRasterisationConfig)
        adaptive_controller_config: GaussianPointAdaptiveController.GaussianPointAdaptiveControllerConfig = field(
            default_factory=GaussianPointAdaptiveController.GaussianPointAdaptiveControllerConfig)
        gaussian_point_cloud_scene_config: GaussianPointCloudScene.PointCloudSceneConfig = field(
            default_factory=GaussianPointCloudScene.PointCloudSceneConfig)
        loss_function_config: LossFunction.LossFunctionConfig = field(
            default_factory=LossFunction.LossFunctionConfig)
        # extensions over the reference
        targets_on_device: bool = True      # targets.TargetStore; False: ImagePoseDataset + the CPU resize (the reference's path)
        sparse_adam: bool = False           # FusedAdam.step(rows=rast.last_touched_rows)
        seed: int = 0                       # of the view order and of the controller's split samples

        @classmethod
        def from_yaml_file(cls, path: str) -> "GaussianPointCloudTrainer.TrainConfig":
            """The config of a YAML file in the reference's format, with or without dataclass_wizard: keys in lisp-case or
            snake_case (a file may mix them), the four nested configs as mappings.  A key no field answers to is ignored and
            listed in config.unknown_keys (nested ones as "adaptive_controller_config.name")."""
            import yaml
            with open(path) as fh:
                data = yaml.safe_load(fh) or {}
            unknown: List[str] = []
            config = _config_from_dict(cls, data, "", unknown)
            config.unknown_keys = unknown
            return config

    def __init__(self, config: TrainConfig, device="cuda", writer=None, pixel_weights: str = "none", mask_erode: int = 0,
                 density: str = "adaptive", mcmc_config: Optional[MCMCConfig] = None, appearance: str = "none",
                 appearance_config: Optional[AppearanceConfig] = None, depth: str = "none", depth_config: Optional[DepthConfig] = None,
                 geometry: Optional[GeometryConfig] = None, bilateral_grid: Optional[BilateralGridConfig] = None,
                 background: str = "none", background_config: Optional[BackgroundConfig] = None, composite_targets: bool = False,
                 filter3d: Optional[Filter3DConfig] = None, pose_refinement: Optional[PoseRefinementConfig] = None,
                 validation_pose_steps: int = 0):
        """device, writer, pixel_weights, mask_erode, density, mcmc_config, appearance and appearance_config are extensions: the GPU to train on; a summary
        writer to use instead of the one make_summary_writer() picks (tensorboard's when it imports, JsonlSummaryWriter
        otherwise); where the per-pixel weights of the loss come from -- "none", "alpha" (the RGBA images' alpha) or "file" (the
        dataset's mask_path column); by how many pixels the mask is shrunk at load (5: no weighted SSIM window sees a masked
        pixel); how the scene grows and shrinks -- "adaptive" (the reference's controller) or "mcmc" (mcmc.MCMCStrategy: a fixed
        budget of Gaussians, mcmc_config.cap_max) -- and the MCMCConfig of the latter (None: the defaults, seeded by config.seed);
        whether every training image gets a learnable colour transform -- "none" or "affine" (appearance.AppearanceTable, in
        self.appearance_table) -- and its AppearanceConfig (None: the defaults, over config.num_iterations); whether the
        dataset's depth maps supervise the rendered depth -- "none", "metric" (metres) or "relative" (relative inverse depth,
        aligned per view) -- and its DepthConfig (None: the defaults, its weight schedule over config.num_iterations); geometry:
        the GeometryConfig of the regularisers on the rendered depth (None: none); bilateral_grid: the BilateralGridConfig of a
        learnable bilateral grid of colour transforms per training image (bilateral.BilateralGridTable, in self.bilateral_table;
        None: none; its schedule runs over config.num_iterations unless it names its own); background: what lies behind the
        splats -- "none", "colour" (background_config.colour), "random" (a colour drawn per step) or "sky" (learnable spherical
        harmonics of the view direction; background.BackgroundModel, in self.background_model) -- its BackgroundConfig (None: the
        defaults, black, its schedule over config.num_iterations), and composite_targets: whether the RGBA training and
        validation pictures are composited over the same background; filter3d: the Filter3DConfig of the 3D smoothing filter
        (filter3d.Filter3D over the training views, in self.filter3d; None: none; its near plane is the rasteriser's unless it
        names its own); pose_refinement: the PoseRefinementConfig of a learnable pose correction per training view
        (pose_table.PoseTable, in self.pose_table; None: none; its schedule runs over config.num_iterations unless it names its
        own), and validation_pose_steps: with it > 0 every validation view is additionally aligned against the frozen scene by
        that many steps of pose_table.refine_pose and measured again (val/psnr_aligned, val/ssim_aligned, val/loss_aligned)"""
        self.config = config
        if pose_refinement is not None:
            pose_refinement.check()
        if int(validation_pose_steps) < 0:
            raise ValueError("validation_pose_steps must be >= 0")
        if validation_pose_steps and background != "none":
            raise ValueError("validation_pose_steps cannot be combined with a background: the aligned render is the bare rasteriser's")
        self.validation_pose_steps = int(validation_pose_steps)
        self.pose_table = None
        if filter3d is not None:
            filter3d.check()
        if background not in ("none",) + _background.KINDS:
            raise ValueError(f'background must be "none", "colour", "random" or "sky", got {background!r}')
        if background == "none" and (background_config is not None or composite_targets):
            raise ValueError('background_config and composite_targets need a background: "colour", "random" or "sky"')
        if background != "none":
            _terms.check_depth_is_rendered(config, f'background="{background}"', "the accumulated alpha and the targets are made on the device")
            if background == "random" and not composite_targets:
                raise ValueError('background="random" needs composite_targets=True: a random colour behind the splats means nothing '
                                 "against pictures that were not composited over it")
            if composite_targets and pixel_weights == "file":
                raise ValueError('composite_targets cannot be combined with pixel_weights="file": the stored fourth channel is the mask, '
                                 "not the pictures' alpha")
            if composite_targets and mask_erode:
                raise ValueError("composite_targets cannot be combined with mask_erode: the pictures are composited with their own alpha")
        self.background, self.composite_targets = background, bool(composite_targets)
        self.background_model = None
        # the extra loss terms, in the order they are summed and logged in; each checks its arguments where it is made
        geometry_terms = _geometry.trainer_terms(geometry, config)
        depth_terms = _depth.trainer_terms(depth, depth_config, config)
        self.terms = depth_terms + geometry_terms
        # The order their autograd nodes on the rendered depth are made in.  Autograd runs the node made last first and adds
        # the gradients up in that order: another order is another float32 sum.
        self._node_order = geometry_terms + depth_terms
        self.geometry = geometry_terms[0].config if geometry_terms else None
        self.depth = depth
        self.depth_config, self.depth_flags = (depth_terms[0].config, depth_terms[0].flags) if depth_terms else (None, 0)
        if appearance not in ("none", "affine"):
            raise ValueError(f'appearance must be "none" or "affine", got {appearance!r}')
        if appearance == "none" and appearance_config is not None:
            raise ValueError('appearance_config needs appearance="affine"')
        if bilateral_grid is not None:
            if appearance == "affine":
                raise ValueError('bilateral_grid cannot be combined with appearance="affine": a grid contains the affine transform')
            bilateral_grid.check()
        self.appearance = appearance
        self.appearance_table = None
        self.bilateral_table = None
        if density not in ("adaptive", "mcmc"):
            raise ValueError(f'density must be "adaptive" or "mcmc", got {density!r}')
        if density == "mcmc" and self.config.sparse_adam:
            raise ValueError('density="mcmc" cannot be combined with sparse_adam=True: its regulariser touches every valid row')
        if density != "mcmc" and mcmc_config is not None:
            raise ValueError('mcmc_config needs density="mcmc"')
        self.density = density
        self.mcmc_config = (mcmc_config or MCMCConfig(seed=int(self.config.seed))) if density == "mcmc" else None
        self.mcmc = None                        # the MCMCStrategy of the running train()
        self.pixel_weights, self.mask_erode = pixel_weights, int(mask_erode)
        self.device = torch.device(device)
        os.makedirs(self.config.summary_writer_log_dir, exist_ok=True)
        if self.config.output_model_dir is None:
            self.config.output_model_dir = self.config.summary_writer_log_dir
        os.makedirs(self.config.output_model_dir, exist_ok=True)
        self.writer = writer if writer is not None else make_summary_writer(self.config.summary_writer_log_dir)
        self.last_validation = None             # (iteration, means) of the last validation()

        self.train_dataset = ImagePoseDataset(dataset_json_path=self.config.train_dataset_json_path)
        self.val_dataset = ImagePoseDataset(dataset_json_path=self.config.val_dataset_json_path)
        self.scene = GaussianPointCloudScene.from_parquet(
            self.config.pointcloud_parquet_path, config=self.config.gaussian_point_cloud_scene_config, device=self.device)
        if self.density == "mcmc":
            self.adaptive_controller = None
            self.rasterisation = GaussianPointCloudRasterisation(config=self.config.rasterisation_config)
        else:
            self.adaptive_controller = GaussianPointAdaptiveController(
                config=self.config.adaptive_controller_config,
                maintained_parameters=GaussianPointAdaptiveController.GaussianPointAdaptiveControllerMaintainedParameters(
                    pointcloud=self.scene.point_cloud,
                    pointcloud_features=self.scene.point_cloud_features,
                    point_invalid_mask=self.scene.point_invalid_mask,
                    point_object_id=self.scene.point_object_id,
                ), seed=self.config.seed)
            self.rasterisation = GaussianPointCloudRasterisation(
                config=self.config.rasterisation_config,
                backward_valid_point_hook=self.adaptive_controller.update,
            )
        self.rasterisation.track_touched_rows = bool(self.config.sparse_adam)
        self.filter3d = None
        if filter3d is not None:
            if filter3d.near is None:
                filter3d = dataclasses.replace(filter3d, near=float(self.config.rasterisation_config.near_plane))
            # one table of the training cameras at factor 1; the rates are taken now, so a validation before train() has them
            self.filter3d = Filter3D(filter3d, self.scene, _filter3d.view_table(self.train_dataset, device=self.device))
        self._filter3d_refinements = 0          # the refinements the filter's rates have seen
        self.loss_function = LossFunction(config=self.config.loss_function_config)
        self.best_psnr_score = 0.

        self.train_targets = self.val_targets = None
        if self.pixel_weights not in ("none", "alpha", "file"):
            raise ValueError(f'pixel_weights must be "none", "alpha" or "file", got {self.pixel_weights!r}')
        self.weighted = self.pixel_weights != "none"
        if self.weighted and not self.config.targets_on_device:
            raise ValueError(f'pixel_weights="{self.pixel_weights}" needs targets_on_device=True: masks are not supported on the '
                             "host target path")
        if self.mask_erode < 0 or (not self.weighted and self.mask_erode):
            raise ValueError('mask_erode must be >= 0, and needs pixel_weights="alpha" or "file"')
        if self.config.targets_on_device:
            mask = dict(mask_source=self.pixel_weights, mask_erode=self.mask_erode) if self.weighted else {}
            if self.composite_targets:
                mask = dict(mask_source="alpha")            # the pictures' alpha: what they are composited with, and the weight if one is asked for
            self.train_targets = TargetStore.from_dataset(self.train_dataset, self.device, **mask)
            self.val_targets = TargetStore.from_dataset(self.val_dataset, self.device, **mask)
        else:
            # batch_size=None: the dataset's items as they are; num_workers=0: no process is started behind an initialised GPU
            self._val_loader = torch.utils.data.DataLoader(self.val_dataset, batch_size=None, shuffle=False, num_workers=0)
        if self.appearance == "affine":
            appearance_config = appearance_config or AppearanceConfig()
            if appearance_config.num_iterations is None:
                appearance_config = dataclasses.replace(appearance_config, num_iterations=max(int(self.config.num_iterations), 1))
            self.appearance_table = AppearanceTable(len(self.train_dataset), self.device, appearance_config)
        if self.background != "none":
            background_config = background_config or BackgroundConfig()
            if background_config.num_iterations is None:
                background_config = dataclasses.replace(background_config, num_iterations=max(int(self.config.num_iterations), 1))
            self.background_model = BackgroundModel(self.background, self.device, background_config)
        if bilateral_grid is not None:
            if bilateral_grid.num_iterations is None:
                bilateral_grid = dataclasses.replace(bilateral_grid, num_iterations=max(int(self.config.num_iterations), 1))
            self.bilateral_table = BilateralGridTable(len(self.train_dataset), self.device, bilateral_grid)
        if pose_refinement is not None:
            if self.filter3d is not None and self.train_targets is None:
                raise ValueError("pose_refinement with filter3d needs targets_on_device=True: the filter's views are made from the "
                                 "store's poses")
            if pose_refinement.num_iterations is None:
                pose_refinement = dataclasses.replace(pose_refinement, num_iterations=max(int(self.config.num_iterations), 1))
            self.pose_table = PoseTable(len(self.train_dataset), self.device, pose_refinement)
        # validation views have no trained correction: the colour-corrected metrics are reported whenever one is trained
        self._colour_corrected = self.appearance_table is not None or self.bilateral_table is not None
        if self.terms:
            # their gradients reach the scene: set on the trainer's own rasteriser, not on the caller's config object
            self.rasterisation.config = copy.copy(self.rasterisation.config)
            self.rasterisation.config.differentiable_depth = True
        for term in self.terms:
            term.load(self.train_dataset, self.val_dataset, self.device)
            if hasattr(term, "bind"):
                term.bind(self)
        # (q, t) of the view being rendered, and whether validation keeps its frames: for a term that renders more over the
        # step's frame than the depth (normals.ConsistencyTerm)
        self.current_pose = None
        self._keep_validation_frame = any(term.name == "consistency" for term in self.terms)
        stores ={term.name: (term.stores["train"], term.stores["val"]) for term in self.terms}
        self.train_depth, self.val_depth = stores.get("depth", (None, None))
        self.train_normals, self.val_normals = stores.get("normal", (None, None))
        # the order the training views are visited in: one seeded permutation per epoch, appended as the run goes
        self._order_generator = torch.Generator().manual_seed(int(self.config.seed))
        self.view_order: List[int] = []

    # ---- targets ----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _downsample_image_and_camera_info(image: torch.Tensor, camera_info: CameraInfo, downsample_factor: int):
        """TRAIN:103-121 on whichever device the image is: the antialiased resize to (H // f, W // f), its crop to multiples of
        16 and the intrinsics divided by f"""
        h_full, w_full, camera_height, camera_width = downsampled_geometry(camera_info.camera_height, camera_info.camera_width,
                                                                           downsample_factor)
        image = resize_antialias(image, (h_full, w_full))
        image = image[:3, :camera_height, :camera_width].contiguous()
        return image, CameraInfo(camera_intrinsics=downsampled_intrinsics(camera_info.camera_intrinsics, downsample_factor),
                                 camera_height=camera_height, camera_width=camera_width, camera_id=camera_info.camera_id)

    def _view_at(self, iteration: int) -> int:
        n = len(self.train_dataset)
        while len(self.view_order) <= iteration:
            self.view_order.extend(torch.randperm(n, generator=self._order_generator).tolist())
        return self.view_order[iteration]

    def _host_target(self, item, downsample_factor: int):
        """the reference's path (TRAIN:149-159): a dataset item, resized on the CPU, then copied to the device"""
        image_gt, q_pointcloud_camera, t_pointcloud_camera, camera_info = item
        if downsample_factor > 1:
            image_gt, camera_info = self._downsample_image_and_camera_info(image_gt, camera_info, downsample_factor)
        camera_info = CameraInfo(camera_intrinsics=camera_info.camera_intrinsics.to(self.device), camera_height=int(camera_info.camera_height),
                                 camera_width=int(camera_info.camera_width), camera_id=camera_info.camera_id)
        return image_gt.to(self.device), q_pointcloud_camera.to(self.device), t_pointcloud_camera.to(self.device), camera_info

    def training_target(self, view: int, downsample_factor: int):
        """-> (image (3,h,w) f32, q (1,4), t (1,3), CameraInfo) of one training view on the device, by the configured path"""
        if self.train_targets is not None:
            return self.train_targets.target(view, downsample_factor)
        return self._host_target(self.train_dataset[view], downsample_factor)

    def _views_from(self, iteration: int):
        """the sampler of the host path's DataLoader: the view of every iteration from `iteration` on, without end"""
        while True:
            yield self._view_at(iteration)
            iteration += 1

    def _target(self, store, host_items, view: int, downsample_factor: int):
        """-> (image, q, t, CameraInfo, pixel weight or None) of a view by the configured path: the split's store, with the
        weight when the loss has one, or (store None) the next item of the host path's loader, which walks the same views"""
        if store is None:
            return self._host_target(next(host_items), downsample_factor) + (None,)
        if self.weighted or self.composite_targets:
            return store.target(view, downsample_factor, with_weight=True)
        return store.target(view, downsample_factor) + (None,)

    def _over_background(self, coef, image_gt, alpha_gt, q_pointcloud_camera, camera_info):
        """-> (the target, the loss's pixel weight): with composite_targets the RGBA picture over the background `coef` in one
        launch (composite_straight's), read from the store's buffer where it lies; the alpha stays the weight only if the loss
        has one"""
        if self.composite_targets:
            with torch.no_grad():
                image_gt = _background.composite_forward(image_gt, alpha_gt, coef.detach(), self.background_model.bands, q_pointcloud_camera,
                                                         camera_info.camera_intrinsics, straight=True)
        return image_gt, (alpha_gt if self.weighted else None)

    def _render_over_background(self, rasterisation_input, coef, **forward):
        """-> (image (3,h,w) composited over `coef`, depth, count): the full forward with its accumulated alpha, then one
        composite node"""
        image_pred, image_depth, pixel_valid_point_count, alpha = self.rasterisation(rasterisation_input, return_accumulated_alpha=True, **forward)
        image_pred = _background.composite(image_pred.permute(2, 0, 1), alpha, coef, self.background_model.bands,
                                           rasterisation_input.q_pointcloud_camera.detach(), rasterisation_input.camera_info.camera_intrinsics)
        return image_pred, image_depth, pixel_valid_point_count

    def _validation_targets(self):
        """-> (image, q, t, CameraInfo, weight or None) of every validation view"""
        host_items = iter(self._val_loader) if self.val_targets is None else None
        for view in range(len(self.val_dataset)):
            yield self._target(self.val_targets, host_items, view, 1)

    def train_image_paths(self) -> List[str]:
        """the image_path of every training view, in the dataset's order: what the rows of the appearance table and the grids of
        the bilateral table belong to"""
        return [str(p) for p in self.train_dataset.df["image_path"].tolist()]

    def _rasterisation_input(self, camera_info, q_pointcloud_camera, t_pointcloud_camera, color_max_sh_band, downsample_factor=1):
        """the scene under the camera; with a 3D filter the features are the filtered ones for a frame at downsample_factor"""
        features = self.scene.point_cloud_features if self.filter3d is None else self.filter3d.features(downsample_factor)
        return GaussianPointCloudRasterisation.GaussianPointCloudRasterisationInput(
            point_cloud=self.scene.point_cloud,
            point_cloud_features=features,
            point_object_id=self.scene.point_object_id,
            point_invalid_mask=self.scene.point_invalid_mask,
            camera_info=camera_info,
            q_pointcloud_camera=q_pointcloud_camera,
            t_pointcloud_camera=t_pointcloud_camera,
            color_max_sh_band=color_max_sh_band,
        )

    def _refinements(self) -> int:
        """the refinements that have changed rows so far, by whichever strategy runs"""
        strategy = self.mcmc if self.mcmc is not None else self.adaptive_controller
        return 0 if strategy is None else int(strategy.refinement_calls)

    def _refresh_filter3d(self, iteration: Optional[int] = None):
        """the filter's rates again: at a multiple of its interval (iteration given), or when a refinement has changed rows
        since they were taken -- new rows have no rate otherwise"""
        if self.filter3d is None:
            return
        due = iteration is not None and iteration % self.filter3d.config.interval == 0
        if due or self._refinements() != self._filter3d_refinements:
            if self.pose_table is not None and any(self.pose_table.steps):
                # (until a correction has taken a step the dataset's own table stands: its rows come from the float64 matrices)
                self.filter3d.views = self._corrected_view_table()
            self.filter3d.refresh()
            self._filter3d_refinements = self._refinements()

    def _corrected_view_table(self):
        """the filter's view table under the training views' corrected poses (PoseTable.corrected: one launch), the intrinsics
        those of the table it replaces.  The rows are made on the host in float64 like the first table's: one host read per
        refresh of the rates."""
        from .utils import quaternion_to_rotation_matrix_torch
        old = self.filter3d.views
        q, t = self.pose_table.corrected(self.train_targets.q, self.train_targets.t)
        q, t = q.cpu().to(torch.float64), t.cpu().to(torch.float64)
        T = torch.eye(4, dtype=torch.float64).repeat(q.shape[0], 1, 1)
        T[:, :3, :3] = quaternion_to_rotation_matrix_torch(q / q.norm(dim=1, keepdim=True))
        T[:, :3, 3] = t
        K = torch.zeros(q.shape[0], 3, 3, dtype=torch.float64)
        fx_fy_cx_cy = old[:, 12:16].cpu().to(torch.float64)
        K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = fx_fy_cx_cy[:, 0], fx_fy_cx_cy[:, 1], fx_fy_cx_cy[:, 2], fx_fy_cx_cy[:, 3], 1.0
        table = torch.from_numpy(_filter3d.view_rows(T.numpy(), K.numpy())).to(self.device)
        table.width, table.height = getattr(old, "width", None), getattr(old, "height", None)
        return table

    def _refining_poses(self, iteration: int) -> bool:
        return self.pose_table is not None and iteration >= self.pose_table.config.start_iteration

    # ---- the loop ---------------------------------------------------------------------------------------------------------
    def train(self):
        config = self.config
        train_items = None
        if self.train_targets is None:
            train_items = iter(torch.utils.data.DataLoader(self.train_dataset, batch_size=None, sampler=self._views_from(0), num_workers=0))
        optimizer = FusedAdam([self.scene.point_cloud_features], lr=config.feature_learning_rate, betas=(0.9, 0.999))
        position_optimizer = FusedAdam([self.scene.point_cloud], lr=config.position_learning_rate, betas=(0.9, 0.999))
        self.optimizer, self.position_optimizer = optimizer, position_optimizer
        if self.density == "mcmc":
            self.mcmc = MCMCStrategy(self.mcmc_config, self.scene, optimizer, position_optimizer)
        downsample_factor = config.initial_downsample_factor
        try:
            from tqdm import tqdm
            iterations = tqdm(range(config.num_iterations), disable=None)
        except Exception:
            iterations = range(config.num_iterations)
        for iteration in iterations:
            if iteration % config.half_downsample_factor_interval == 0 and iteration > 0 and downsample_factor > 1:
                downsample_factor = downsample_factor // 2
            optimizer.zero_grad()
            position_optimizer.zero_grad()
            self._refresh_filter3d(iteration)

            view = self._view_at(iteration)
            image_gt, q_pointcloud_camera, t_pointcloud_camera, camera_info, pixel_weight = self._target(
                self.train_targets, train_items, view, downsample_factor)
            if self._refining_poses(iteration):
                # the view's correction on the right of the dataset's pose; its gradient is written into the table's row.  (The
                # sky's gradient to the pose is not taken: the background is handed the composed pose detached.)
                q_pointcloud_camera, t_pointcloud_camera = _pose_table.compose(q_pointcloud_camera, t_pointcloud_camera,
                                                                               self.pose_table.row(view))
                self.current_pose = (q_pointcloud_camera.detach(), t_pointcloud_camera.detach())
            else:
                self.current_pose = (q_pointcloud_camera, t_pointcloud_camera)
            rasterisation_input =self._rasterisation_input(
                camera_info, q_pointcloud_camera, t_pointcloud_camera,
                color_max_sh_band=color_max_sh_band_at(iteration, config.increase_color_max_sh_band_interval),
                downsample_factor=downsample_factor)
            if self.background_model is not None:
                # the step's background: behind the splats, and behind the RGBA target if that is composited
                background_coef = self.background_model.coef_for_step()
                image_gt, pixel_weight = self._over_background(background_coef, image_gt, pixel_weight, self.current_pose[0], camera_info)
                image_pred, image_depth, pixel_valid_point_count = self._render_over_background(rasterisation_input, background_coef)
            else:
                image_pred, image_depth, pixel_valid_point_count = self.rasterisation(rasterisation_input)
                # hxwx3->3xhxw, read where it lies; the clamp to [0, 1] runs inside the loss kernels
                image_pred = image_pred.permute(2, 0, 1)
            if self.appearance_table is not None:
                # the view's colour transform, in the rasteriser's layout: the loss reads the corrected image where it lies
                image_pred = _appearance.apply(image_pred, self.appearance_table.row(view))
            if self.bilateral_table is not None:
                # the view's grid, sliced at every pixel; same layout, so the loss reads the corrected image where it lies
                image_pred = _bilateral.slice(image_pred, self.bilateral_table.row(view))
            loss, l1_loss, ssim_loss = self.loss_function(
                image_pred,
                image_gt,
                point_invalid_mask=self.scene.point_invalid_mask,
                pointcloud_features=self.scene.point_cloud_features,
                clamp_predicted=True,
                pixel_weight=pixel_weight)          # None: the unweighted loss
            values = {term: term.value("train", view, downsample_factor, image_depth, image_gt, camera_info, pixel_weight)
                      for term in self._node_order if iteration >= term.start_iteration}
            total = loss
            for term in self.terms:
                if values.get(term) is not None:
                    total = total + term.weight_at(iteration) * values[term]
            total.backward()
            if self.bilateral_table is not None:
                # tv_weight * d tv / d grid of this view's grid, added to the gradient the backward wrote; the value stays on the device
                table = self.bilateral_table
                _bilateral.tv(table.grids[view], weight=table.config.tv_weight, grad_grid=table.grad, value=table.tv_value)
            if self.mcmc is not None:
                self.mcmc.before_step(iteration)
            rows = self.rasterisation.last_touched_rows if config.sparse_adam else None
            optimizer.step(rows=rows)
            position_optimizer.step(rows=rows)
            if self.background_model is not None:
                self.background_model.step(iteration)           # "sky" alone moves
            if self.appearance_table is not None:
                self.appearance_table.step(view, iteration)
            if self.bilateral_table is not None:
                self.bilateral_table.step(view, iteration)
            if self._refining_poses(iteration):
                self.pose_table.step(view, iteration)

            if self.mcmc is not None:
                self.mcmc.after_step(iteration, position_optimizer.lr)       # the rate this iteration stepped with
            if iteration % config.position_learning_rate_decay_interval == 0:
                position_optimizer.lr *= config.position_learning_rate_decay_rate
            if self.adaptive_controller is not None:
                self.adaptive_controller.refinement()
            self._refresh_filter3d()            # a refinement of this iteration: its new rows get their rates now

            # (the reference reads loss.item() every iteration to pick "problematic" images for its image log; there is no
            # image log here, so the loss is read -- and the host waits for the device -- only where it is logged)
            if iteration % config.log_loss_interval == 0:
                loss_value = loss.item()
                self.writer.add_scalar("train/loss", loss_value, iteration)
                self.writer.add_scalar("train/l1 loss", l1_loss.item(), iteration)
                self.writer.add_scalar("train/ssim loss", ssim_loss.item(), iteration)
                if self.bilateral_table is not None:
                    self.writer.add_scalar("train/bilateral_tv", self.bilateral_table.tv_value.item(), iteration)     # the one host read
                for term in self.terms:
                    if values.get(term) is not None:
                        for tag, value in term.train_scalars(values[term].terms.tolist()):       # one read per term
                            self.writer.add_scalar(tag, value, iteration)
                if config.print_metrics_to_console:
                    print(f"train_iteration={iteration};")
                    print(f"train_loss={loss_value};")
                    print(f"train_l1_loss={l1_loss.item()};")
                    print(f"train_ssim_loss={ssim_loss.item()};")
            if iteration % config.log_metrics_interval == 0:
                self.writer.add_scalar("value/num_valid_points", int((self.scene.point_invalid_mask == 0).sum().item()), iteration)
                # (a view whose mask is empty has no PSNR or SSIM: nothing is logged for it)
                if pixel_weight is None or bool((pixel_weight > 0).any()):
                    _, psnr_score, ssim_loss_clamped = self._metrics(torch.clamp(image_pred.detach(), 0, 1), image_gt, pixel_weight)
                    ssim_score = 1.0 - ssim_loss_clamped
                    self.writer.add_scalar("train/psnr", psnr_score.item(), iteration)
                    self.writer.add_scalar("train/ssim", ssim_score.item(), iteration)
                    if config.print_metrics_to_console:
                        print(f"train_psnr={psnr_score.item()};")
                        print(f"train_psnr_{iteration}={psnr_score.item()};")
                        print(f"train_ssim={ssim_score.item()};")
                        print(f"train_ssim_{iteration}={ssim_score.item()};")
            del image_gt, q_pointcloud_camera, t_pointcloud_camera, camera_info, rasterisation_input, image_pred, loss, l1_loss, ssim_loss
            del pixel_weight, image_depth, values, total
            self.current_pose = None
            # they use 7000 in paper, it's hard to set a interval so hard code it here (TRAIN:274)
            if (iteration % config.val_interval == 0 and iteration != 0) or iteration == 7000 or iteration == 5000:
                self.validation(iteration)
        if hasattr(self.writer, "flush"):
            self.writer.flush()

    @staticmethod
    def _weighted_mse(image_pred, image_gt, pixel_weight):
        """sum w (x - y)^2 / (3 sum w), w as the loss has it (anything not > 0 is 0, by selection); plain torch.  The callers
        leave out a view whose weights are all zero: it has no mean."""
        w = torch.where(pixel_weight > 0, pixel_weight, torch.zeros_like(pixel_weight))
        squared = torch.where(w > 0, w * (image_pred - image_gt) ** 2, torch.zeros_like(image_pred))
        return squared.sum() / (3 * w.sum())

    def _metrics(self, image_pred, image_gt, pixel_weight=None):
        """-> (loss, PSNR, SSIM loss) of a predicted image in [0, 1], device scalars: PSNR = 10 log10(1 / mse); SSIM is 1 - the
        SSIM loss, the third term of the loss (pytorch_msssim.ssim's definition, in its kernels).  With a weight: the weighted
        loss and the mse over the weighted pixels.  (The SSIM loss and not the SSIM: the train log subtracts in float32, the
        validation the host's number from 1, and both keep their last bit.)"""
        with torch.no_grad():
            loss, _, ssim_loss = self.loss_function(image_pred, image_gt, pixel_weight=pixel_weight)     # None: the unweighted loss
            mse = torch.mean((image_pred - image_gt) ** 2) if pixel_weight is None else self._weighted_mse(image_pred, image_gt, pixel_weight)
            return loss, 10 * torch.log10(1.0 / mse), ssim_loss

    def validation(self, iteration):
        """TRAIN:342-423: every validation view at band 3 and full resolution; the means of loss, PSNR, SSIM and of the
        rasteriser's time by device events are logged, the scene written as scene_<iteration>.parquet and, when the mean PSNR is
        the best so far, as best_scene.parquet.  -> the means, as a dict.  With pixel weights a view whose mask is empty is left
        out of every mean: it has no weighted pixel to measure."""
        with torch.no_grad():
            sums = dict(loss=0.0, psnr=0.0, ssim=0.0, inference_time=0.0)
            if self._colour_corrected:
                sums.update(loss_cc=0.0, psnr_cc=0.0, ssim_cc=0.0)
            if self.validation_pose_steps > 0:
                sums.update(loss_aligned=0.0, psnr_aligned=0.0, ssim_aligned=0.0)
            count = 0
            total_terms, term_count = {term: 0.0 for term in self.terms}, {term: 0 for term in self.terms}
            for val_view, (image_gt, q_pointcloud_camera, t_pointcloud_camera, camera_info, pixel_weight) in enumerate(self._validation_targets()):
                if self.background_model is not None:
                    image_gt, pixel_weight = self._over_background(self.background_model.coef, image_gt, pixel_weight, q_pointcloud_camera,
                                                                   camera_info)
                if pixel_weight is not None and not bool((pixel_weight > 0).any()):
                    continue
                start_event = torch.cuda.Event(enable_timing=True)
                end_event = torch.cuda.Event(enable_timing=True)
                rasterisation_input = self._rasterisation_input(camera_info, q_pointcloud_camera, t_pointcloud_camera, color_max_sh_band=3)
                self.current_pose = (q_pointcloud_camera, t_pointcloud_camera)
                start_event.record()
                if self.background_model is not None:
                    image_pred, image_depth, pixel_valid_point_count = self._render_over_background(
                        rasterisation_input, self.background_model.coef, keep_frame=self._keep_validation_frame)
                else:
                    image_pred, image_depth, pixel_valid_point_count = self.rasterisation(rasterisation_input, keep_frame=self._keep_validation_frame)
                end_event.record()
                torch.cuda.synchronize()
                sums["inference_time"] += start_event.elapsed_time(end_event)
                # (composited: already 3xhxw)
                image_pred = torch.clamp(image_pred, 0, 1) if self.background_model is not None else torch.clamp(image_pred, 0, 1).permute(2, 0, 1)
                images = {"": image_pred}
                if self._colour_corrected:
                    # a validation view has no trained transform: the best affine map onto its ground truth, then the same metrics
                    fitted = _appearance.fit_affine(image_pred, image_gt, pixel_weight)
                    images["_cc"] = torch.clamp(_appearance.apply_forward(image_pred, fitted), 0, 1)
                for suffix, image in images.items():
                    loss, psnr_score, ssim_loss = self._metrics(image, image_gt, pixel_weight)
                    sums["loss" + suffix] += loss.item()
                    sums["psnr" + suffix] += psnr_score.item()
                    sums["ssim" + suffix] += 1.0 - ssim_loss.item()
                for term in self.terms:
                    # (for depth="relative" the aligned loss: the fit is part of the forward)
                    value = term.value("val", val_view, 1, image_depth, image_gt, camera_info, pixel_weight)
                    if value is not None:
                        total_terms[term] += value.item()
                        term_count[term] += 1
                if self.validation_pose_steps > 0:
                    # a validation view has no trained correction, and a scene trained with refined poses may have moved against
                    # the dataset's frame: align the view against the frozen scene, then the same metrics (the BARF / nerfstudio
                    # protocol).  Last: these renders replace the view's frame.
                    with torch.enable_grad():
                        q_aligned, t_aligned, _ = _pose_table.refine_pose(self.rasterisation, rasterisation_input, image_gt,
                                                                          self.validation_pose_steps, pixel_weight=pixel_weight,
                                                                          loss_function=self.loss_function)
                    aligned = self.rasterisation(dataclasses.replace(rasterisation_input, q_pointcloud_camera=q_aligned,
                                                                     t_pointcloud_camera=t_aligned))[0]
                    loss, psnr_score, ssim_loss = self._metrics(torch.clamp(aligned, 0, 1).permute(2, 0, 1), image_gt, pixel_weight)
                    sums["loss_aligned"] += loss.item()
                    sums["psnr_aligned"] += psnr_score.item()
                    sums["ssim_aligned"] += 1.0 - ssim_loss.item()
                count += 1
            count = max(count, 1)
            means = {name: total / count for name, total in sums.items()}
            means.update({f"{term.name}_loss": total_terms[term] / n_views for term, n_views in term_count.items() if n_views})
            for name, value in means.items():
                self.writer.add_scalar(f"val/{name}", value, iteration)
            if self.config.print_metrics_to_console:
                print(f"val_loss={means['loss']};")
                print(f"val_psnr={means['psnr']};")
                print(f"val_psnr_{iteration}={means['psnr']};")
                print(f"val_ssim={means['ssim']};")
                print(f"val_ssim_{iteration}={means['ssim']};")
                print(f"val_inference_time={means['inference_time']};")
            self.scene.to_parquet(os.path.join(self.config.output_model_dir, f"scene_{iteration}.parquet"))
            if self.appearance_table is not None:
                self.appearance_table.save(os.path.join(self.config.output_model_dir, f"appearance_{iteration}.pt"), self.train_image_paths())
            if self.bilateral_table is not None:
                self.bilateral_table.save(os.path.join(self.config.output_model_dir, f"bilateral_{iteration}.pt"), self.train_image_paths())
            if self.background_model is not None:
                self.background_model.save(os.path.join(self.config.output_model_dir, f"background_{iteration}.pt"))
            if self.filter3d is not None:
                self.filter3d.save(os.path.join(self.config.output_model_dir, f"filter3d_{iteration}.pt"))
            if self.pose_table is not None:
                self.pose_table.save(os.path.join(self.config.output_model_dir, f"poses_{iteration}.pt"), self.train_image_paths())
            if means["psnr"] > self.best_psnr_score:
                self.best_psnr_score = means["psnr"]
                self.scene.to_parquet(os.path.join(self.config.output_model_dir, "best_scene.parquet"))
                if self.appearance_table is not None:
                    self.appearance_table.save(os.path.join(self.config.output_model_dir, "best_appearance.pt"), self.train_image_paths())
                if self.bilateral_table is not None:
                    self.bilateral_table.save(os.path.join(self.config.output_model_dir, "best_bilateral.pt"), self.train_image_paths())
                if self.background_model is not None:
                    self.background_model.save(os.path.join(self.config.output_model_dir, "best_background.pt"))
                if self.filter3d is not None:
                    self.filter3d.save(os.path.join(self.config.output_model_dir, "best_filter3d.pt"))
                if self.pose_table is not None:
                    self.pose_table.save(os.path.join(self.config.output_model_dir, "best_poses.pt"), self.train_image_paths())
            if hasattr(self.writer, "flush"):
                self.writer.flush()
            self.last_validation = (iteration, means)
            return means
