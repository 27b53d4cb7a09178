"""GPU (-m gpu): bilateral grids through GaussianPointCloudTrainer(config, bilateral_grid=BilateralGridConfig(...)) on the 64x96
views of tests/trainer_util.py's dataset: None is the loop as it was, the first iteration with a grid is the step written out by
hand (slice, loss, backward, tv added, Adam on that view's grid alone), the grid cannot be combined with the affine table, and
grids trained on pictures with a different radial vignette planted per view -- which no single 3x4 transform represents --
take it up better than the affine table does.  GS_BILATERAL_MARGINS_OUT=<file> records the quality run's numbers
(profiles/bilateral_margins.json holds a run)."""
import json
import os

import numpy as np
import PIL.Image
import pytest
import torch

import trainer_util as TU
from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast, bilateral
from taichi_3d_gaussian_splatting_amd.appearance import AppearanceConfig
from taichi_3d_gaussian_splatting_amd.bilateral import BilateralGridConfig, BilateralGridTable
from taichi_3d_gaussian_splatting_amd.GaussianPointAdaptiveController import GaussianPointAdaptiveController
from taichi_3d_gaussian_splatting_amd.GaussianPointCloudScene import GaussianPointCloudScene
from taichi_3d_gaussian_splatting_amd.GaussianPointTrainer import GaussianPointCloudTrainer, JsonlSummaryWriter
from taichi_3d_gaussian_splatting_amd.ImagePoseDataset import ImagePoseDataset
from taichi_3d_gaussian_splatting_amd.LossFunction import LossFunction
from taichi_3d_gaussian_splatting_amd.optim import FusedAdam
from taichi_3d_gaussian_splatting_amd.targets import TargetStore
from test_gpu_trainer import hand_written_loop

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_TRAIN = len(TU.TRAIN_VIEWS)
# Planted per training view, on the uint8 data: value * (1 - k r^2), r the distance from the picture's centre, 1 at the corners.
# A gain only darkens, so no channel can saturate.  The strengths differ between the views, so the scene cannot take them up.
VIGNETTES = (0.55, 0.15, 0.45, 0.25, 0.6, 0.35)
SCHEDULE = dict(TU.SMOKE)           # 120 iterations: 20 steps per view
# Fixed before the runs were first compared.  20 Adam steps per view move a value by at most 20 lr, and a corner has to come
# down by up to 0.6, so both tables get lr 0.03 -> 0.01 (the affine one too: it is not held back by a smaller rate).  The grid
# is 5x5 over the 32x48 to 64x96 pictures -- a vignette is smooth -- with the two luminance levels a grid must have; tv_weight is
# the default.
RATES = dict(lr=0.03, lr_final=0.01)
GRID = dict(grid_x=5, grid_y=5, grid_l=2, **RATES)


def vignette_gain(k, H, W):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    cy, cx = (H - 1) / 2.0, (W - 1) / 2.0
    r2 = ((y - cy) ** 2 + (x - cx) ** 2) / (cy ** 2 + cx ** 2)
    return 1.0 - k * r2


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """trainer_util's dataset from the perturbed scene: `plain`; `vignetted`: the training pictures under the planted vignettes
    (validation untouched)"""
    root = tmp_path_factory.mktemp("bilateral_data")
    base = TU.write_dataset(root, DEV, initial=TU.perturbed(TU.ground_truth_scene()))
    records = json.load(open(base["paths"]["train"]))
    assert len(records) == N_TRAIN == len(VIGNETTES)
    os.makedirs(root / "vignetted", exist_ok=True)
    altered = []
    for r, k in zip(records, VIGNETTES):
        image = np.array(PIL.Image.open(r["image_path"])).astype(np.float64)
        value = image[:, :, :3] * vignette_gain(k, image.shape[0], image.shape[1])[:, :, None]
        path = str(root / "vignetted" / os.path.basename(r["image_path"]))
        PIL.Image.fromarray(np.round(value).astype(np.uint8)).save(path)
        altered.append(dict(r, image_path=path))
    paths = dict(base["paths"], train=str(root / "train_vignetted.json"))
    json.dump(altered, open(paths["train"], "w"))
    return {"plain": base, "vignetted": dict(paths=paths, images=base["images"])}


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


def test_none_is_the_loop_as_it_was(data, tmp_path):
    n_it, band_interval, decay_interval, rate = 3, 2, 2, 0.9
    trainer = make_trainer(data["plain"], tmp_path, num_iterations=n_it, initial_downsample_factor=1, bilateral_grid=None,
                           increase_color_max_sh_band_interval=band_interval, position_learning_rate_decay_interval=decay_interval,
                           position_learning_rate_decay_rate=rate, position_learning_rate=1e-4, log_loss_interval=1, seed=3)
    assert trainer.bilateral_table is None
    trainer.train()
    scene, _, _ = hand_written_loop(data["plain"], trainer.config, trainer.view_order, n_it, band_interval, decay_interval, rate, False, seed=3)
    assert torch.equal(trainer.scene.point_cloud, scene.point_cloud)
    assert torch.equal(trainer.scene.point_cloud_features, scene.point_cloud_features)
    means = trainer.validation(n_it)
    assert set(means) == {"loss", "psnr", "ssim", "inference_time"} and logged(trainer, "train/bilateral_tv") == []
    assert not any("bilateral" in f for f in os.listdir(trainer.config.output_model_dir))
    with pytest.raises(ValueError, match="affine"):
        make_trainer(data["plain"], tmp_path / "x", appearance="affine", bilateral_grid=BilateralGridConfig())
    with pytest.raises(ValueError, match="grid_l"):
        make_trainer(data["plain"], tmp_path / "y", bilateral_grid=BilateralGridConfig(grid_l=9))
    # it needs nothing else: the host target path takes it too
    host = make_trainer(data["plain"], tmp_path / "z", num_iterations=1, targets_on_device=False, bilateral_grid=BilateralGridConfig(grid_x=4, grid_y=3, grid_l=2))
    host.train()
    assert sum(host.bilateral_table.steps) == 1


def test_first_iteration_with_a_grid_is_the_manual_step(data, tmp_path):
    factor = 2
    grid_config = BilateralGridConfig(grid_x=6, grid_y=4, grid_l=3)
    trainer = make_trainer(data["vignetted"], tmp_path, num_iterations=1, initial_downsample_factor=factor, bilateral_grid=grid_config,
                           log_loss_interval=1, log_metrics_interval=10 ** 6, position_learning_rate=1e-4, seed=3)
    table = trainer.bilateral_table
    assert table.num_views == N_TRAIN and table.config.num_iterations == 1 and grid_config.num_iterations is None
    assert table.grids.shape == (N_TRAIN, 4, 6, 3, 12) and table.grad.shape == (4, 6, 3, 12)
    trainer.train()
    torch.cuda.synchronize()
    view = trainer.view_order[0]

    config = trainer.config
    scene = GaussianPointCloudScene.from_parquet(data["vignetted"]["paths"]["cloud"], config=config.gaussian_point_cloud_scene_config, device=DEV)
    controller = GaussianPointAdaptiveController(
        config=config.adaptive_controller_config,
        maintained_parameters=GaussianPointAdaptiveController.GaussianPointAdaptiveControllerMaintainedParameters(
            pointcloud=scene.point_cloud, pointcloud_features=scene.point_cloud_features,
            point_invalid_mask=scene.point_invalid_mask, point_object_id=scene.point_object_id), seed=3)
    rast = Rast(Rast.GaussianPointCloudRasterisationConfig(), backward_valid_point_hook=controller.update)
    loss_fn = LossFunction(LossFunction.LossFunctionConfig())
    of = FusedAdam([scene.point_cloud_features], lr=config.feature_learning_rate)
    op = FusedAdam([scene.point_cloud], lr=config.position_learning_rate)
    manual = BilateralGridTable(N_TRAIN, DEV, BilateralGridConfig(grid_x=6, grid_y=4, grid_l=3, num_iterations=1))
    gt, q, t, info = TargetStore.from_dataset(ImagePoseDataset(data["vignetted"]["paths"]["train"]), DEV).target(view, factor)
    img = rast(Rast.GaussianPointCloudRasterisationInput(
        point_cloud=scene.point_cloud, point_cloud_features=scene.point_cloud_features, point_object_id=scene.point_object_id,
        point_invalid_mask=scene.point_invalid_mask, camera_info=info, q_pointcloud_camera=q, t_pointcloud_camera=t,
        color_max_sh_band=0))[0]
    row = manual.row(view)
    corrected = bilateral.slice(img.permute(2, 0, 1), row)                      # 1
    assert torch.equal(corrected, img.detach().permute(2, 0, 1))               # the identity grid is exact
    assert corrected.stride() == img.permute(2, 0, 1).stride()
    L, l1, ld = loss_fn(corrected, gt, point_invalid_mask=scene.point_invalid_mask, pointcloud_features=scene.point_cloud_features,
                        clamp_predicted=True)                                   # 2
    L.backward()                                                                # 3
    data_grad = manual.grad.clone()
    value = bilateral.tv(manual.grids[view], weight=manual.config.tv_weight, grad_grid=manual.grad)     # 4
    assert float(value) == 0.0 and torch.equal(manual.grad, data_grad)         # an identity grid has no variation yet
    of.step(); op.step(); manual.step(view, 0)                                  # 5
    controller.refinement()
    torch.cuda.synchronize()
    assert logged(trainer, "train/loss") == [(0, float(L.item()))] and logged(trainer, "train/l1 loss") == [(0, float(l1.item()))]
    assert logged(trainer, "train/bilateral_tv") == [(0, 0.0)]
    assert torch.equal(trainer.scene.point_cloud, scene.point_cloud) and torch.equal(trainer.scene.point_cloud_features, scene.point_cloud_features)
    for name in ("grids", "grad", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(table, name), getattr(manual, name)), name
    assert table.steps == manual.steps and table.steps[view] == 1 and sum(table.steps) == 1
    # every other view's grid and moments are untouched, bit for bit
    others = [i for i in range(N_TRAIN) if i != view]
    fresh = BilateralGridTable(N_TRAIN, DEV, grid_config)
    assert torch.equal(table.grids[others], fresh.grids[others])
    assert not table.exp_avg[others].any() and not table.exp_avg_sq[others].any()
    assert not torch.equal(table.grids[view], fresh.grids[view]) and bool(table.grad.any())

    # a second step of the same view: now the grid varies, and the tv term is in the gradient the Adam step takes
    trainer2 = make_trainer(data["vignetted"], tmp_path / "two", num_iterations=N_TRAIN + 1, initial_downsample_factor=factor,
                            bilateral_grid=grid_config, log_loss_interval=1, log_metrics_interval=10 ** 6, position_learning_rate=1e-4, seed=3)
    trainer2.train()
    tv_log = logged(trainer2, "train/bilateral_tv")
    again = [i for i, v in enumerate(trainer2.view_order[:N_TRAIN + 1]) if v in trainer2.view_order[:i]]
    assert [s for s, _ in tv_log] == list(range(N_TRAIN + 1)) and all(v == 0.0 for s, v in tv_log if s not in again)
    assert again == [N_TRAIN] and all(v > 0.0 for s, v in tv_log if s in again)


def test_grids_take_up_planted_vignettes_better_than_the_affine_table(data, tmp_path):
    """Three runs of trainer_util.SMOKE (120 iterations, 20 per view) on the vignetted pictures, the same initial scene and
    seed: (a) no correction, (b) appearance="affine", (c) a 5x5x2 grid per view; the two tables at the same learning rates.
    The condition: the last epoch's train/l1 of (c) is below both others'.

    Measured on an MI355X (profiles/bilateral_margins.json, written by this test under GS_BILATERAL_MARGINS_OUT): last-epoch
    train/l1 0.01183 (a), 0.01006 (b), 0.00795 (c), the geometric mean of (b) and (c) 0.00894; val/psnr 31.27 (a), 34.33 (b),
    34.60 (c); val/psnr_cc 34.55 (b), 34.99 (c)."""
    runs = {}
    for name, kwargs in (("plain", {}), ("affine", dict(appearance="affine", appearance_config=AppearanceConfig(**RATES))),
                         ("grid", dict(bilateral_grid=BilateralGridConfig(**GRID)))):
        trainer = make_trainer(data["vignetted"], tmp_path / name, regularise=False, log_loss_interval=1, log_metrics_interval=10 ** 6, seed=0,
                               **SCHEDULE, **kwargs)
        trainer.train()
        iteration, means = trainer.last_validation
        assert iteration == SCHEDULE["val_interval"]
        l1 = logged(trainer, "train/l1 loss")
        assert [s for s, _ in l1] == list(range(SCHEDULE["num_iterations"]))
        runs[name] = (trainer, means, float(np.mean([v for _, v in l1[-N_TRAIN:]])))
    (tp, vp, lp), (ta, va, la), (tg, vg, lg) = runs["plain"], runs["affine"], runs["grid"]
    assert tp.view_order == ta.view_order == tg.view_order
    assert sorted(tg.view_order[-N_TRAIN:]) == list(range(N_TRAIN))            # the last epoch sees every view once
    print(f"last-epoch train/l1: plain {lp:.5f}, affine {la:.5f}, grid {lg:.5f} (geometric mean of grid and affine {np.sqrt(lg * la):.5f})")
    print(f"val/psnr: plain {vp['psnr']:.3f}, affine {va['psnr']:.3f}, grid {vg['psnr']:.3f}; val/psnr_cc: affine {va['psnr_cc']:.3f}, grid {vg['psnr_cc']:.3f}")
    out = os.environ.get("GS_BILATERAL_MARGINS_OUT")
    if out:
        record = json.load(open(out)) if os.path.exists(out) else {}
        record["trainer_vignettes"] = dict(
            schedule=SCHEDULE, vignettes=list(VIGNETTES), grid=GRID, affine=RATES,
            last_epoch_train_l1=dict(plain=lp, affine=la, grid=lg), geometric_mean_of_grid_and_affine=float(np.sqrt(lg * la)),
            val_psnr=dict(plain=vp["psnr"], affine=va["psnr"], grid=vg["psnr"]), val_psnr_cc=dict(affine=va["psnr_cc"], grid=vg["psnr_cc"]),
            last_bilateral_tv=logged(tg, "train/bilateral_tv")[-1][1])
        with open(out, "w") as fh:
            json.dump(record, fh, indent=1)
    assert lg < la and lg < lp
    # validation as with the affine table: uncorrected views, and the colour-corrected metrics beside the plain ones
    assert set(vg) == set(va) == {"loss", "psnr", "ssim", "inference_time", "loss_cc", "psnr_cc", "ssim_cc"} and set(vp) == set(vg) - {"loss_cc", "psnr_cc", "ssim_cc"}
    assert all(np.isfinite(x) for x in vg.values()) and 0 < vg["ssim_cc"] <= 1
    tv_log = logged(tg, "train/bilateral_tv")
    assert len(tv_log) == SCHEDULE["num_iterations"] and tv_log[-1][1] > 0.0 and all(np.isfinite(v) for _, v in tv_log)
    # Scene and grids are determined only up to a common factor per place, so what a grid means is its difference from the
    # other views': the view under the strongest vignette darkens its corners against its centre more than the one under the weakest
    grids = tg.bilateral_table.grids
    gain = grids[..., [0, 5, 10]].mean(dim=(3, 4))                                  # (V,Gy,Gx): mean diagonal gain over levels and channels
    ratio = gain[:, [0, 0, -1, -1], [0, -1, 0, -1]].mean(dim=1) / gain[:, 2, 2]
    assert float(ratio[int(np.argmax(VIGNETTES))]) < float(ratio[int(np.argmin(VIGNETTES))])
    # the files of the validation: the table beside every scene, and they load back
    model = tg.config.output_model_dir
    k = SCHEDULE["val_interval"]
    assert os.path.exists(os.path.join(model, f"scene_{k}.parquet")) and os.path.exists(os.path.join(model, f"bilateral_{k}.pt"))
    assert os.path.exists(os.path.join(model, "best_scene.parquet")) and os.path.exists(os.path.join(model, "best_bilateral.pt"))
    assert not any(f.startswith("appearance") or f.startswith("best_appearance") for f in os.listdir(model))
    loaded, paths = BilateralGridTable.load(os.path.join(model, f"bilateral_{k}.pt"), DEV)
    assert torch.equal(loaded.grids, grids) and loaded.steps == tg.bilateral_table.steps == [SCHEDULE["num_iterations"] // N_TRAIN] * N_TRAIN
    assert paths == [r["image_path"] for r in json.load(open(data["vignetted"]["paths"]["train"]))]
    assert (loaded.config.grid_x, loaded.config.grid_y, loaded.config.grid_l) == (5, 5, 2)
