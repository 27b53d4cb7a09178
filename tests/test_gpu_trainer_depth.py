"""GPU (-m gpu): depth supervision through GaussianPointCloudTrainer(config, depth="metric" | "relative") on the 64x96 views
of tests/trainer_util.py's dataset with the depth files of tests/depth_trainer_util.py: "none" is the loop as it was, a
supervised run ends with a smaller depth error than the same run without, relative inverse depth with a scale and shift per
view trains and logs its fit, the combination with masks runs, and what cannot work is refused."""
import json
import os

import numpy as np
import PIL.Image
import pytest
import torch

import depth_trainer_util as DU
import trainer_util as TU
from taichi_3d_gaussian_splatting_amd.depth import DepthConfig
from taichi_3d_gaussian_splatting_amd.GaussianPointTrainer import GaussianPointCloudTrainer, JsonlSummaryWriter

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_TRAIN = len(TU.TRAIN_VIEWS)
MASK_BOX = (8, 56, 10, 80)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """`plain`: trainer_util's dataset from the perturbed scene; `metric`: with the ground truth's depth in 16-bit PNGs;
    `relative`: with a / Z + b per view instead, a and b different for every view"""
    root = tmp_path_factory.mktemp("depth_data")
    base = TU.write_dataset(root, DEV, initial=TU.perturbed(TU.ground_truth_scene()))
    metric = DU.add_depth(base, root, DEV)
    relative = DU.add_depth(base, root, DEV, transform=lambda view, z: (1.5 + 0.25 * view) / np.where(z > 0, z, 1.0) + 0.05 * (view + 1),
                            name="relative")
    return dict(plain=base, metric=metric, relative=relative)


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


def test_the_depth_files_hold_the_ground_truth(data):
    metric = data["metric"]
    for view, z in metric["depth"].items():
        stored = np.array(PIL.Image.open(os.path.join(os.path.dirname(metric["paths"]["train"]), "depth", f"view_{view}.png")))
        assert stored.dtype == np.uint16 and np.array_equal(stored, metric["stored"][view])
        assert np.array_equal(stored == 0, z == 0) and 0.05 < (z == 0).mean() < 0.95          # holes and surface both
        assert np.abs(stored * metric["depth_scale"] - z)[z > 0].max() <= 0.5 * metric["depth_scale"] * 1.001
    assert max(int(s.max()) for s in metric["stored"].values()) == DU.U16_TOP
    records = json.load(open(metric["paths"]["train"]))
    assert all(r["depth_scale"] == metric["depth_scale"] for r in records)


def test_none_leaves_the_run_bit_identical(data, tmp_path):
    """depth="none" on a dataset that has depth files against a trainer built without the argument"""
    runs = []
    for name, kwargs in (("without", {}), ("none", dict(depth="none"))):
        trainer = make_trainer(data["metric"], tmp_path / name, num_iterations=4, initial_downsample_factor=2, log_loss_interval=1,
                               log_metrics_interval=10 ** 6, position_learning_rate=1e-4, seed=3, **kwargs)
        assert trainer.depth == "none" and trainer.train_depth is None and trainer.val_depth is None and trainer.depth_config is None
        assert not getattr(trainer.rasterisation.config, "differentiable_depth", False)
        trainer.train()
        runs.append(trainer)
    a, b = runs
    assert torch.equal(a.scene.point_cloud, b.scene.point_cloud) and torch.equal(a.scene.point_cloud_features, b.scene.point_cloud_features)
    for tag in ("train/loss", "train/l1 loss", "train/ssim loss"):
        assert logged(a, tag) == logged(b, tag) and len(logged(a, tag)) == 4
    assert logged(b, "train/depth loss") == []
    assert set(b.validation(4)) == {"loss", "psnr", "ssim", "inference_time"}


def test_supervision_lowers_the_depth_error(data, tmp_path):
    """The same seeded run of trainer_util.SMOKE with depth="metric" and without: the mean masked |D - Z| over the validation
    views, measured here for both, is lower with supervision.  (tools/bench_depth_loss.py writes both values and both
    validation PSNRs to profiles/depth_margins.json.)  Measured on an MI355X: 0.1531 without, 0.0401 with; val/psnr 39.03
    without, 36.81 with."""
    runs = DU.supervised_and_plain_runs(data["metric"], tmp_path, DEV)
    none, metric = runs["none"], runs["metric"]
    print(f"validation mean |D - Z|: without {none['depth_error']:.5f}, with depth=\"metric\" {metric['depth_error']:.5f}; "
          f"val/psnr without {none['psnr']:.3f}, with {metric['psnr']:.3f}")
    assert none["trainer"].view_order == metric["trainer"].view_order
    assert metric["trainer"].rasterisation.config.differentiable_depth is True
    assert not getattr(metric["trainer"].config.rasterisation_config, "differentiable_depth", False)      # the caller's config is left alone
    assert "depth_loss" in metric["means"] and "depth_loss" not in none["means"] and np.isfinite(metric["means"]["depth_loss"])
    steps = [s for s, _ in logged(metric["trainer"], "train/depth loss")]
    assert steps == list(range(0, TU.SMOKE["num_iterations"], 10)) and logged(metric["trainer"], "train/depth scale") == []
    assert all(np.isfinite(v) and v >= 0 for _, v in logged(metric["trainer"], "train/depth loss"))
    assert not torch.equal(none["trainer"].scene.point_cloud, metric["trainer"].scene.point_cloud)
    assert metric["depth_error"] < none["depth_error"]


def test_relative_depth_trains_and_logs_its_fit(data, tmp_path):
    """Targets a / Z + b with another a, b per view.  Measured on an MI355X: aligned val/depth_loss 0.01012 at iteration 0,
    0.00335 at iteration 119 (with the default schedule, 1 -> 0.01 within the 120 iterations, 0.01093: the colour term alone
    raises it again)."""
    trainer = make_trainer(data["relative"], tmp_path, regularise=False, seed=0, log_loss_interval=10, depth="relative",
                           depth_config=DepthConfig(**DU.SHORT_RUN), **TU.SMOKE)
    assert trainer.depth_flags == 1 | 8                        # x = 1 / D, the target as stored, aligned
    before = trainer.validation(0)
    trainer.train()
    iteration, after = trainer.last_validation
    assert iteration == TU.SMOKE["val_interval"]
    scales, shifts = logged(trainer, "train/depth scale"), logged(trainer, "train/depth shift")
    assert len(scales) == len(shifts) == TU.SMOKE["num_iterations"] // 10
    assert all(np.isfinite(v) for _, v in scales + shifts) and all(v > 0 for _, v in scales)
    # the planted map is y = a / Z + b: the fit of x = 1 / D onto it has s near 1 / a, within the range of the views' a
    a = [1.5 + 0.25 * v for v in TU.TRAIN_VIEWS]
    assert all(0.5 / max(a) < v < 2.0 / min(a) for _, v in scales)
    print(f"aligned val/depth_loss: iteration 0 {before['depth_loss']:.6f}, iteration {iteration} {after['depth_loss']:.6f}")
    assert np.isfinite(after["depth_loss"]) and after["depth_loss"] < before["depth_loss"]


def test_masks_and_depth_run_together(data, tmp_path):
    root = tmp_path / "masked"
    os.makedirs(root)
    mask = np.zeros((TU.H, TU.W), np.uint8)
    mask[MASK_BOX[0]:MASK_BOX[1], MASK_BOX[2]:MASK_BOX[3]] = 255
    PIL.Image.fromarray(mask, mode="L").save(root / "mask.png")
    paths = dict(data["metric"]["paths"])
    for split in ("train", "val"):
        records = [dict(r, mask_path=str(root / "mask.png")) for r in json.load(open(paths[split]))]
        paths[split] = str(root / f"{split}.json")
        json.dump(records, open(paths[split], "w"))
    trainer = make_trainer(dict(paths=paths), tmp_path / "run", num_iterations=2, initial_downsample_factor=1, pixel_weights="file",
                           depth="metric", log_loss_interval=1, log_metrics_interval=1, seed=3)
    trainer.train()
    means = trainer.validation(2)
    assert all(np.isfinite(v) for v in means.values()) and "depth_loss" in means
    for t in (trainer.scene.point_cloud, trainer.scene.point_cloud_features):
        assert bool(torch.isfinite(t.detach()).all())
    assert len(logged(trainer, "train/depth loss")) == 2
    # the mask reaches the depth term: outside the box nothing is selected
    view = trainer.view_order[0]
    _, _, _, _, weight = trainer.train_targets.target(view, 1, with_weight=True)
    z, wt = trainer.train_depth.target(view, 1, 0.5)
    from taichi_3d_gaussian_splatting_amd import depth as depth_module
    rendered = torch.full_like(z, 2.0)
    both = depth_module.depth_loss(rendered, z, wt, weight).terms[4].item()
    one = depth_module.depth_loss(rendered, z, wt).terms[4].item()
    inside = float(((wt > 0) & (z > 0) & (weight > 0)).sum().item())
    assert both == inside < one


def test_what_cannot_work_is_refused(data, tmp_path):
    with pytest.raises(ValueError, match="depth"):
        make_trainer(data["metric"], tmp_path / "a", depth="lidar")
    with pytest.raises(ValueError, match="depth_config"):
        make_trainer(data["metric"], tmp_path / "b", depth_config=DepthConfig())
    with pytest.raises(ValueError, match="targets_on_device"):
        make_trainer(data["metric"], tmp_path / "c", depth="metric", targets_on_device=False)
    with pytest.raises(ValueError, match="depth_path"):
        make_trainer(data["plain"], tmp_path / "d", depth="metric")
    with pytest.raises(ValueError, match="space"):
        make_trainer(data["relative"], tmp_path / "e", depth="relative", depth_config=DepthConfig(space="depth"))
    config = TU.train_config(data["metric"]["paths"], tmp_path / "f")
    config.rasterisation_config.rgb_only = True
    with pytest.raises(ValueError, match="rgb_only"):
        GaussianPointCloudTrainer(config, device=DEV, depth="metric")
    with pytest.raises(ValueError, match="min_coverage"):
        make_trainer(data["metric"], tmp_path / "g", depth="metric", depth_config=DepthConfig(min_coverage=2.0))
