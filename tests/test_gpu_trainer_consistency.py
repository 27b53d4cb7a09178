"""GPU (-m gpu): the normal-consistency term through GaussianPointCloudTrainer(config, geometry=GeometryConfig(consistency_weight=...))
on the 64x96 views of tests/trainer_util.py's dataset: a weight of 0 is the loop as it was, the first iteration is the step
written out by hand, the tags are logged, what cannot work is refused, the command-line flags reach the config, the renderer
writes the rendered Gaussian normals, and a run with the term ends with Gaussian normals closer to the normals of the rendered
depth than the same run without."""
import json
import os
import runpy
import sys

import numpy as np
import PIL.Image
import pytest
import torch

import geometry_trainer_util as GU
import trainer_util as TU
from taichi_3d_gaussian_splatting_amd import geometry, normals
from taichi_3d_gaussian_splatting_amd.geometry import GeometryConfig
from taichi_3d_gaussian_splatting_amd.GaussianPointTrainer import GaussianPointCloudTrainer, JsonlSummaryWriter

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The weight of the 120-iteration run, fixed before the two runs were first compared: the term is a mean of 1 - cos, of order 0.1
# to 1 on a scene whose Gaussians were never asked to be flat, against a colour loss of 0.018 at iteration 0 (geometry_trainer_util).
SHORT_RUN = dict(consistency_weight=0.1)
MARGINS = os.path.join(ROOT, "profiles", "normal_consistency_margins.json")


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    root = tmp_path_factory.mktemp("consistency_data")
    return TU.write_dataset(root, DEV, initial=TU.perturbed(TU.ground_truth_scene()))


def make_trainer(data, out_dir, regularise=True, **kwargs):
    """kwargs that TrainConfig has are config overrides, the others constructor arguments"""
    fields = {f for f in GaussianPointCloudTrainer.TrainConfig.__dataclass_fields__}
    config = TU.train_config(data["paths"], out_dir, **{k: v for k, v in kwargs.items() if k in fields})
    config.loss_function_config.enable_regularization = regularise
    return GaussianPointCloudTrainer(config, device=DEV, writer=JsonlSummaryWriter(config.summary_writer_log_dir),
                                     **{k: v for k, v in kwargs.items() if k not in fields})


def logged(trainer, tag):
    trainer.writer.flush()
    return [(r["step"], r["value"]) for r in JsonlSummaryWriter.read(trainer.writer.path) if r["tag"] == tag]


def validation_consistency_angle(trainer, min_length=0.5, max_rel_jump=0.1):
    """the mean over the validation views of the mean angle, in degrees, between the rendered Gaussian normals (normalised where
    at least min_length long) and geometry.depth_normals of the rendered depth, over the pixels where both exist"""
    angles = []
    with torch.no_grad():
        for i in range(len(TU.VAL_VIEWS)):
            _, q, t, info = trainer.val_targets.target(i, 1)[:4]
            _, depth, _ = trainer.rasterisation(trainer._rasterisation_input(info, q, t, color_max_sh_band=3), keep_frame=True)
            g = normals.unit_normals(normals.rendered_normals(trainer.rasterisation, trainer.scene, (q, t)), min_length).double()
            n = geometry.depth_normals(depth, info.camera_intrinsics, max_rel_jump).double()
            both = (n != 0).any(dim=0) & (g != 0).any(dim=0)
            assert int(both.sum()) > 100
            cos = (n * g).sum(dim=0)[both].clamp(-1.0, 1.0)
            angles.append(float(torch.rad2deg(torch.acos(cos)).mean()))
    return float(np.mean(angles))


def test_zero_weight_and_none_leave_the_run_bit_identical(data, tmp_path):
    """geometry=None against a trainer built without the argument, and consistency_weight=0 beside a positive smoothness against
    the same config without the field"""
    common = dict(num_iterations=4, initial_downsample_factor=2, log_loss_interval=1, log_metrics_interval=10 ** 6, position_learning_rate=1e-4, seed=3)
    runs = {}
    for name, kwargs in (("without", {}), ("none", dict(geometry=None)), ("smooth", dict(geometry=GeometryConfig(smooth_weight=0.5))),
                         ("smooth_zero", dict(geometry=GeometryConfig(smooth_weight=0.5, consistency_weight=0.0, consistency_min_length=0.25)))):
        trainer = make_trainer(data, tmp_path / name, **common, **kwargs)
        trainer.train()
        runs[name] = trainer
    for a, b in (("without", "none"), ("smooth", "smooth_zero")):
        a, b = runs[a], runs[b]
        assert torch.equal(a.scene.point_cloud, b.scene.point_cloud) and torch.equal(a.scene.point_cloud_features, b.scene.point_cloud_features)
        for tag in ("train/loss", "train/l1 loss", "train/ssim loss", "train/smooth loss"):
            assert logged(a, tag) == logged(b, tag)
        assert logged(b, "train/consistency loss") == [] and [type(t).__name__ for t in b.terms] == [type(t).__name__ for t in a.terms]
        assert b._keep_validation_frame is False
        assert a.validation(4) .keys() == b.validation(4).keys() and "consistency_loss" not in b.last_validation[1]
    assert not torch.equal(runs["none"].scene.point_cloud, runs["smooth"].scene.point_cloud)
    assert not getattr(runs["none"].rasterisation.config, "differentiable_depth", False)


def test_first_step_with_the_term_is_the_manual_step(data, tmp_path):
    """One trainer iteration with the consistency term alone at 32x48 against the same step written out by hand: the frame of the
    step's forward, rendered_normals over it, normal_consistency of the rendered depth and them, loss + w * term.  Gradients
    and logged values are equal bit for bit."""
    import copy
    from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast
    from taichi_3d_gaussian_splatting_amd.GaussianPointAdaptiveController import GaussianPointAdaptiveController
    from taichi_3d_gaussian_splatting_amd.GaussianPointCloudScene import GaussianPointCloudScene
    from taichi_3d_gaussian_splatting_amd.ImagePoseDataset import ImagePoseDataset
    from taichi_3d_gaussian_splatting_amd.LossFunction import LossFunction
    from taichi_3d_gaussian_splatting_amd.targets import TargetStore
    factor = 2
    g = GeometryConfig(consistency_weight=0.1, consistency_min_length=0.3)
    trainer = make_trainer(data, tmp_path / "run", num_iterations=1, initial_downsample_factor=factor, geometry=g, log_loss_interval=1,
                           log_metrics_interval=10 ** 6, val_interval=10 ** 6, seed=3)
    assert [t.name for t in trainer.terms] == ["consistency"] and trainer._node_order == trainer.terms and trainer._keep_validation_frame
    assert trainer.rasterisation.config.differentiable_depth is True
    assert not getattr(trainer.config.rasterisation_config, "differentiable_depth", False)
    trainer.train()
    torch.cuda.synchronize()
    view = trainer.view_order[0]
    paths, config = data["paths"], trainer.config
    scene = GaussianPointCloudScene.from_parquet(paths["cloud"], config=config.gaussian_point_cloud_scene_config, device=DEV)
    controller = GaussianPointAdaptiveController(
        config=config.adaptive_controller_config,
        maintained_parameters=GaussianPointAdaptiveController.GaussianPointAdaptiveControllerMaintainedParameters(
            pointcloud=scene.point_cloud, pointcloud_features=scene.point_cloud_features,
            point_invalid_mask=scene.point_invalid_mask, point_object_id=scene.point_object_id), seed=3)
    rast_config = copy.copy(config.rasterisation_config)
    rast_config.differentiable_depth = True
    rast = Rast(rast_config, backward_valid_point_hook=controller.update)
    loss_fn = LossFunction(config.loss_function_config)
    targets = TargetStore.from_dataset(ImagePoseDataset(paths["train"]), DEV)
    gt, q, t, info = targets.target(view, factor)
    img, rendered, _ = rast(Rast.GaussianPointCloudRasterisationInput(
        point_cloud=scene.point_cloud, point_cloud_features=scene.point_cloud_features, point_object_id=scene.point_object_id,
        point_invalid_mask=scene.point_invalid_mask, camera_info=info, q_pointcloud_camera=q, t_pointcloud_camera=t, color_max_sh_band=0))
    L, l1, ld = loss_fn(img.permute(2, 0, 1), gt, point_invalid_mask=scene.point_invalid_mask, pointcloud_features=scene.point_cloud_features,
                        clamp_predicted=True, pixel_weight=None)
    Rn = normals.rendered_normals(rast, scene, (q, t))
    term = normals.normal_consistency(rendered, Rn, info.camera_intrinsics, None, g.consistency_max_rel_jump, g.consistency_min_length)
    (L + g.consistency_weight * term).backward()
    torch.cuda.synchronize()
    assert term.terms[0].item() > 0 and term.terms[2].item() > 50
    for tag, value in (("train/loss", L.item()), ("train/l1 loss", l1.item()), ("train/ssim loss", ld.item()),
                       ("train/consistency loss", term.terms[0].item())):
        assert logged(trainer, tag) == [(0, float(value))], tag
    assert torch.equal(trainer.scene.point_cloud.grad, scene.point_cloud.grad) and bool(scene.point_cloud.grad.any())
    assert torch.equal(trainer.scene.point_cloud_features.grad, scene.point_cloud_features.grad)
    # the term reached the quaternions: without it their gradient differs
    plain = make_trainer(data, tmp_path / "plain", num_iterations=1, initial_downsample_factor=factor, log_loss_interval=1,
                         log_metrics_interval=10 ** 6, val_interval=10 ** 6, seed=3)
    plain.train()
    assert not torch.equal(plain.scene.point_cloud_features.grad[:, :4], scene.point_cloud_features.grad[:, :4])
    # validation logs the term and keeps its frames only for it
    means = trainer.validation(1)
    assert np.isfinite(means["consistency_loss"]) and means["consistency_loss"] > 0 and logged(trainer, "val/consistency_loss") == [(1, means["consistency_loss"])]
    assert "consistency_loss" not in plain.validation(1) and plain._keep_validation_frame is False


def test_start_iteration_and_the_other_terms(data, tmp_path):
    trainer = make_trainer(data, tmp_path / "both", num_iterations=4, initial_downsample_factor=2, log_loss_interval=1, log_metrics_interval=10 ** 6,
                           seed=3, geometry=GeometryConfig(smooth_weight=0.5, consistency_weight=0.05, start_iteration=2))
    assert [t.name for t in trainer.terms] == ["smooth", "consistency"] == [t.name for t in trainer._node_order]
    trainer.train()
    assert [s for s, _ in logged(trainer, "train/consistency loss")] == [2, 3] == [s for s, _ in logged(trainer, "train/smooth loss")]
    assert all(np.isfinite(v) and v >= 0 for _, v in logged(trainer, "train/consistency loss"))
    assert set(trainer.validation(4)) == {"loss", "psnr", "ssim", "inference_time", "smooth_loss", "consistency_loss"}
    for t in (trainer.scene.point_cloud, trainer.scene.point_cloud_features):
        assert bool(torch.isfinite(t.detach()).all())


def test_what_cannot_work_is_refused(data, tmp_path):
    with pytest.raises(ValueError, match="consistency_weight"):
        make_trainer(data, tmp_path / "a", geometry=GeometryConfig())
    with pytest.raises(ValueError, match="consistency_weight must be finite and >= 0"):
        make_trainer(data, tmp_path / "b", geometry=GeometryConfig(consistency_weight=-1.0))
    with pytest.raises(ValueError, match="consistency_min_length must be finite and > 0"):
        make_trainer(data, tmp_path / "c", geometry=GeometryConfig(consistency_weight=0.1, consistency_min_length=0.0))
    with pytest.raises(ValueError, match="consistency_max_rel_jump"):
        make_trainer(data, tmp_path / "d", geometry=GeometryConfig(consistency_weight=0.1, consistency_max_rel_jump=float("nan")))
    with pytest.raises(ValueError, match="targets_on_device"):
        make_trainer(data, tmp_path / "e", geometry=GeometryConfig(consistency_weight=0.1), targets_on_device=False)
    config = TU.train_config(data["paths"], tmp_path / "f")
    config.rasterisation_config.rgb_only = True
    with pytest.raises(ValueError, match="rgb_only"):
        GaussianPointCloudTrainer(config, device=DEV, geometry=GeometryConfig(consistency_weight=0.1))
    with pytest.raises(RuntimeError, match="bind"):
        normals.ConsistencyTerm(GeometryConfig(consistency_weight=0.1)).value("train", 0, 1, None, None, None, None)


def test_the_command_line_flags_reach_the_config(tmp_path, monkeypatch):
    """gaussian_point_train.py run in this process with the trainer class replaced by one that records its arguments"""
    from taichi_3d_gaussian_splatting_amd import GaussianPointTrainer as module
    seen = {}

    class Recorder:
        TrainConfig = GaussianPointCloudTrainer.TrainConfig

        def __init__(self, config, **kwargs):
            seen.update(kwargs)

        def train(self):
            seen["trained"] = True

    monkeypatch.setattr(module, "GaussianPointCloudTrainer", Recorder)
    yaml_path = tmp_path / "config.yaml"
    yaml_path.write_text("num-iterations: 3\n")
    script = os.path.join(ROOT, "gaussian_point_train.py")
    monkeypatch.setattr(sys, "argv", [script, "--train_config", str(yaml_path), "--normal_consistency", "0.07", "--consistency_min_length", "0.4",
                                      "--consistency_start", "500"])
    runpy.run_path(script, run_name="__main__")
    g = seen["geometry"]
    assert seen["trained"] and isinstance(g, GeometryConfig)
    assert (g.consistency_weight, g.consistency_min_length, g.start_iteration, g.consistency_max_rel_jump) == (0.07, 0.4, 500, 0.1)
    assert g.smooth_weight == 0.0 and g.normal_weight == 0.0
    g.check()
    seen.clear()
    monkeypatch.setattr(sys, "argv", [script, "--train_config", str(yaml_path)])
    runpy.run_path(script, run_name="__main__")
    assert seen["geometry"] is None
    monkeypatch.setattr(sys, "argv", [script, "--train_config", str(yaml_path), "--consistency_start", "5"])
    with pytest.raises(SystemExit):
        runpy.run_path(script, run_name="__main__")


def test_the_renderer_writes_the_rendered_gaussian_normals(data, tmp_path):
    """--normals_source gaussians: files that decode to unit normals facing the camera; the default is the depth's normal"""
    from taichi_3d_gaussian_splatting_amd.GaussianPointRenderer import GaussianPointRenderer
    from taichi_3d_gaussian_splatting_amd.ImagePoseDataset import ImagePoseDataset
    from taichi_3d_gaussian_splatting_amd.targets import TargetStore
    targets = TargetStore.from_dataset(ImagePoseDataset(data["paths"]["val"]), DEV)
    renderer = GaussianPointRenderer(GaussianPointRenderer.GaussianPointRendererConfig(data["paths"]["cloud"], torch.eye(4).unsqueeze(0), device=DEV,
                                                                                      image_height=TU.H, image_width=TU.W))
    assert renderer.write_normals(tmp_path / "g", targets=targets, source="gaussians", min_length=0.5) == len(TU.VAL_VIEWS)
    assert renderer.write_normals(tmp_path / "d", targets=targets) == len(TU.VAL_VIEWS)
    with pytest.raises(ValueError, match="source"):
        renderer.write_normals(tmp_path / "x", targets=targets, source="mesh")
    fx, fy, cx, cy = GU.intrinsics()
    yy, xx = np.mgrid[0:TU.H, 0:TU.W].astype(np.float64)
    rays = np.stack([(xx + 0.5 - cx) / fx, (yy + 0.5 - cy) / fy, np.ones_like(xx)], axis=2)
    for i in range(len(TU.VAL_VIEWS)):
        coded = np.array(PIL.Image.open(tmp_path / "g" / f"normal_{i:03d}.png"))
        assert coded.dtype == np.uint8 and coded.shape == (TU.H, TU.W, 3)
        has = coded.any(axis=2)
        n = coded.astype(np.float64) / 127.5 - 1.0
        assert 0.05 < has.mean() < 1.0
        assert np.abs(np.linalg.norm(n, axis=2)[has] - 1.0).max() < 3.0 / 255                       # unit, to the 8-bit step
        # facing the camera: every Gaussian's normal has n . p <= 0 for its own centre; a pixel's ray differs from those of the
        # centres blended into it by the Gaussians' extent, so nearly all, not all
        assert ((n * rays).sum(axis=2)[has] < 0).mean() > 0.95
        other = np.array(PIL.Image.open(tmp_path / "d" / f"normal_{i:03d}.png"))
        assert other.shape == coded.shape and not np.array_equal(other, coded)


def test_the_term_brings_the_gaussian_normals_to_the_depth_normals(data, tmp_path):
    """The same seeded run of trainer_util.SMOKE with SHORT_RUN and without (the baseline is the run without the term: the loop as
    it was): the mean angle over the validation views between the rendered Gaussian normals and the normals of the rendered
    depth.  Measured on an MI355X (profiles/normal_consistency_margins.json): 67.39 degrees without, 37.13 with; val/psnr 39.03
    without, 32.54 with (reported, not asserted: at this weight the term costs 6.5 dB on this scene of separate blobs).  The test
    asserts half the measured gap of 30.26 degrees."""
    runs = {}
    for name, kwargs in (("none", {}), ("consistency", dict(geometry=GeometryConfig(**SHORT_RUN)))):
        config = TU.train_config(data["paths"], tmp_path / name, seed=0, log_loss_interval=10, **TU.SMOKE)
        config.loss_function_config.enable_regularization = False
        trainer = GaussianPointCloudTrainer(config, device=DEV, writer=JsonlSummaryWriter(config.summary_writer_log_dir), **kwargs)
        trainer.train()
        iteration, means = trainer.last_validation
        assert iteration == TU.SMOKE["val_interval"]
        runs[name] = dict(angle=validation_consistency_angle(trainer), psnr=float(means["psnr"]), means=means, trainer=trainer)
    none, con = runs["none"], runs["consistency"]
    print(f"consistency angle: without {none['angle']:.4f} degrees, with the term {con['angle']:.4f}; val/psnr without {none['psnr']:.3f}, "
          f"with {con['psnr']:.3f}")
    assert none["trainer"].view_order == con["trainer"].view_order
    assert "consistency_loss" in con["means"] and "consistency_loss" not in none["means"]
    assert [s for s, _ in logged(con["trainer"], "train/consistency loss")] == list(range(0, TU.SMOKE["num_iterations"], 10))
    for t in (con["trainer"].scene.point_cloud, con["trainer"].scene.point_cloud_features):
        assert bool(torch.isfinite(t.detach()).all())
    measured = json.load(open(MARGINS))
    gap = measured["none"]["angle_degrees"] - measured["consistency"]["angle_degrees"]
    assert gap > 0
    assert con["angle"] <= none["angle"] - 0.5 * gap
