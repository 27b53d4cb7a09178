"""GPU (-m gpu): exposure compensation through GaussianPointCloudTrainer(config, appearance="affine") on the 64x96 views of
tests/trainer_util.py's dataset: "none" is the loop as it was, the first "affine" iteration is the step written out by hand,
a table trained on images with planted gains and offsets takes the difference between the views up, the combinations with
masks and with the fixed-budget strategy run, and the files the trainer writes are the ones the render script reads."""
import json
import os
import subprocess
import sys

import numpy as np
import PIL.Image
import pytest
import torch

import trainer_util as TU
from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast, appearance
from taichi_3d_gaussian_splatting_amd.appearance import AppearanceConfig, AppearanceTable
from taichi_3d_gaussian_splatting_amd.GaussianPointAdaptiveController import GaussianPointAdaptiveController
from taichi_3d_gaussian_splatting_amd.GaussianPointCloudScene import GaussianPointCloudScene
from taichi_3d_gaussian_splatting_amd.GaussianPointRenderer import GaussianPointRenderer
from taichi_3d_gaussian_splatting_amd.GaussianPointTrainer import GaussianPointCloudTrainer, JsonlSummaryWriter
from taichi_3d_gaussian_splatting_amd.ImagePoseDataset import ImagePoseDataset
from taichi_3d_gaussian_splatting_amd.LossFunction import LossFunction
from taichi_3d_gaussian_splatting_amd.mcmc import MCMCConfig
from taichi_3d_gaussian_splatting_amd.optim import FusedAdam
from taichi_3d_gaussian_splatting_amd.targets import TargetStore
from test_gpu_trainer import hand_written_loop

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_TRAIN = len(TU.TRAIN_VIEWS)
# Planted per training view, on the uint8 data: value * gain + offset, rounded.  Gains within 0.85 .. 1.15 and offsets within
# +-10 / 255, chosen on the low side of both ranges' products so that no channel can saturate whatever a picture holds:
# 255 * 0.96 + 10 < 255.5 at the top, and a black background stays at or above 0 because no offset is negative.
GAINS = (0.85, 0.96, 0.88, 0.94, 0.86, 0.92)
OFFSETS = (10, 0, 2, 8, 4, 6)
PAIR = (0, 1)                       # the two views whose recovered gain ratio is looked at: the most different gains
MASK_BOX = (8, 56, 10, 80)
SCHEDULE = dict(TU.SMOKE)           # 120 iterations: 20 steps per view
APPEARANCE = dict(lr=0.01, lr_final=0.001)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """trainer_util's dataset from the perturbed scene: `plain`; `altered`: the training pictures with the planted gains and
    offsets (validation untouched); `masked` / `corrupted`: four plain training views with a mask file, once as they are,
    once with noise where the mask is 0"""
    root = tmp_path_factory.mktemp("appearance_data")
    base = TU.write_dataset(root, DEV, initial=TU.perturbed(TU.ground_truth_scene()))
    records = {split: json.load(open(base["paths"][split])) for split in ("train", "val")}
    assert len(records["train"]) == N_TRAIN == len(GAINS) == len(OFFSETS)
    out = {"plain": base}

    def variant(name, train_records, val_records=None):
        paths = dict(base["paths"], train=str(root / f"train_{name}.json"), val=str(root / f"val_{name}.json"))
        json.dump(train_records, open(paths["train"], "w"))
        json.dump(val_records if val_records is not None else records["val"], open(paths["val"], "w"))
        out[name] = dict(paths=paths, images=base["images"])

    os.makedirs(root / "altered", exist_ok=True)
    altered = []
    for r, gain, offset in zip(records["train"], GAINS, OFFSETS):
        value = np.array(PIL.Image.open(r["image_path"])).astype(np.float64) * gain + offset
        assert value.min() >= 0.0 and value.max() <= 255.0, "a channel would saturate"
        path = str(root / "altered" / os.path.basename(r["image_path"]))
        PIL.Image.fromarray(np.round(value).astype(np.uint8)).save(path)
        altered.append(dict(r, image_path=path))
    variant("altered", altered)

    mask = np.zeros((TU.H, TU.W), np.uint8)
    mask[MASK_BOX[0]:MASK_BOX[1], MASK_BOX[2]:MASK_BOX[3]] = 255
    PIL.Image.fromarray(mask, mode="L").save(root / "mask.png")
    rng = np.random.default_rng(7)
    os.makedirs(root / "corrupted", exist_ok=True)
    masked = {split: [dict(r, mask_path=str(root / "mask.png")) for r in records[split][:4]] for split in ("train", "val")}
    corrupted = {}
    for split in ("train", "val"):
        corrupted[split] = []
        for r in masked[split]:
            image = np.array(PIL.Image.open(r["image_path"]))
            image[mask == 0] = rng.integers(0, 256, (int((mask == 0).sum()), 3))
            path = str(root / "corrupted" / os.path.basename(r["image_path"]))
            PIL.Image.fromarray(image).save(path)
            corrupted[split].append(dict(r, image_path=path))
    variant("masked", masked["train"], masked["val"])
    variant("corrupted", corrupted["train"], corrupted["val"])
    return out


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
    trainer = make_trainer(data["plain"], tmp_path, num_iterations=n_it, initial_downsample_factor=1, appearance="none",
                           increase_color_max_sh_band_interval=band_interval, position_learning_rate_decay_interval=decay_interval,
                           position_learning_rate_decay_rate=rate, position_learning_rate=1e-4, seed=3)
    assert trainer.appearance == "none" and trainer.appearance_table is None
    trainer.train()
    scene, _, _ = hand_written_loop(data["plain"], trainer.config, trainer.view_order, n_it, band_interval, decay_interval, rate, False, seed=3)
    assert torch.equal(trainer.scene.point_cloud, scene.point_cloud)
    assert torch.equal(trainer.scene.point_cloud_features, scene.point_cloud_features)
    means = trainer.validation(n_it)
    assert set(means) == {"loss", "psnr", "ssim", "inference_time"}
    assert not any(f.startswith("appearance") or f.startswith("best_appearance") for f in os.listdir(trainer.config.output_model_dir))
    with pytest.raises(ValueError, match="appearance"):
        make_trainer(data["plain"], tmp_path / "x", appearance="bilateral")
    with pytest.raises(ValueError, match="appearance_config"):
        make_trainer(data["plain"], tmp_path / "y", appearance_config=AppearanceConfig())
    assert not hasattr(GaussianPointCloudTrainer.TrainConfig(), "appearance")


def test_first_affine_iteration_is_the_manual_step(data, tmp_path):
    factor = 2
    trainer = make_trainer(data["altered"], tmp_path, num_iterations=1, initial_downsample_factor=factor, appearance="affine",
                           log_loss_interval=1, log_metrics_interval=10 ** 6, position_learning_rate=1e-4, seed=3)
    table = trainer.appearance_table
    assert table.num_views == N_TRAIN and table.config.num_iterations == 1 and (table.config.lr, table.config.lr_final) == (0.01, 0.001)
    trainer.train()
    torch.cuda.synchronize()
    view = trainer.view_order[0]

    config = trainer.config
    scene = GaussianPointCloudScene.from_parquet(data["altered"]["paths"]["cloud"], config=config.gaussian_point_cloud_scene_config, device=DEV)
    controller = GaussianPointAdaptiveController(
        config=config.adaptive_controller_config,
        maintained_parameters=GaussianPointAdaptiveController.GaussianPointAdaptiveControllerMaintainedParameters(
            pointcloud=scene.point_cloud, pointcloud_features=scene.point_cloud_features,
            point_invalid_mask=scene.point_invalid_mask, point_object_id=scene.point_object_id), seed=3)
    rast = Rast(Rast.GaussianPointCloudRasterisationConfig(), backward_valid_point_hook=controller.update)
    loss_fn = LossFunction(LossFunction.LossFunctionConfig())
    of = FusedAdam([scene.point_cloud_features], lr=config.feature_learning_rate)
    op = FusedAdam([scene.point_cloud], lr=config.position_learning_rate)
    manual = AppearanceTable(N_TRAIN, DEV, AppearanceConfig(num_iterations=1))
    gt, q, t, info = TargetStore.from_dataset(ImagePoseDataset(data["altered"]["paths"]["train"]), DEV).target(view, factor)
    img = rast(Rast.GaussianPointCloudRasterisationInput(
        point_cloud=scene.point_cloud, point_cloud_features=scene.point_cloud_features, point_object_id=scene.point_object_id,
        point_invalid_mask=scene.point_invalid_mask, camera_info=info, q_pointcloud_camera=q, t_pointcloud_camera=t,
        color_max_sh_band=0))[0]
    row = manual.row(view)
    assert row.detach().cpu().tolist() == list(appearance.IDENTITY)
    corrected = appearance.apply(img.permute(2, 0, 1), row)
    assert torch.equal(corrected, img.detach().permute(2, 0, 1))               # 1 x + 0 + 0 + 0: the identity is exact
    L, l1, ld = loss_fn(corrected, gt, point_invalid_mask=scene.point_invalid_mask, pointcloud_features=scene.point_cloud_features,
                        clamp_predicted=True)
    L.backward()
    of.step(); op.step(); manual.step(view, 0)
    controller.refinement()
    torch.cuda.synchronize()
    assert logged(trainer, "train/loss") == [(0, float(L.item()))] and logged(trainer, "train/l1 loss") == [(0, float(l1.item()))]
    assert torch.equal(trainer.scene.point_cloud, scene.point_cloud) and torch.equal(trainer.scene.point_cloud_features, scene.point_cloud_features)
    for name in ("transforms", "grad", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(table, name), getattr(manual, name)), name
    assert table.steps == manual.steps and table.steps[view] == 1 and sum(table.steps) == 1
    others = [i for i in range(N_TRAIN) if i != view]
    assert table.transforms[others].cpu().tolist() == [list(appearance.IDENTITY)] * len(others)
    assert bool((table.transforms[view] != torch.tensor(appearance.IDENTITY, device=DEV)).any()) and bool(table.grad[view].any())


def test_a_trained_table_takes_up_planted_gains_and_offsets(data, tmp_path):
    """Three runs of trainer_util.SMOKE (120 iterations, 20 per view), the same initial scene and seed: (a) plain images
    without a table, (b) altered images without, (c) altered images with one.

    Measured on an MI355X with SCHEDULE = trainer_util.SMOKE and the default AppearanceConfig (lr 0.01 -> 0.001; no need to
    raise it): last-epoch train/l1 0.00596 (a), 0.01638 (b), 0.00632 (c), midpoint 0.01117; val/psnr 39.03 (a), 35.63 (b),
    37.51 (c) and val/psnr_cc 38.56 (c); gain ratio of views 1 and 0 recovered 1.0368, planted 1.1294, the planted gains 0.11
    apart (the offsets are recovered to 0.039 of a planted 10 / 255 = 0.0392: most of what 20 steps move goes there first)."""
    runs = {}
    for name, images, kwargs in (("a", "plain", {}), ("b", "altered", {}),
                                 ("c", "altered", dict(appearance="affine", appearance_config=AppearanceConfig(**APPEARANCE)))):
        trainer = make_trainer(data[images], tmp_path / name, regularise=False, log_loss_interval=1, log_metrics_interval=10 ** 6, seed=0,
                               **SCHEDULE, **kwargs)
        trainer.train()
        iteration, means = trainer.last_validation
        assert iteration == SCHEDULE["val_interval"]
        l1 = logged(trainer, "train/l1 loss")
        assert [s for s, _ in l1] == list(range(SCHEDULE["num_iterations"]))
        last_epoch = float(np.mean([v for _, v in l1[-N_TRAIN:]]))
        runs[name] = (trainer, means, last_epoch)
    (ta, va, la), (tb, vb, lb), (tc, vc, lc) = runs["a"], runs["b"], runs["c"]
    assert ta.view_order == tb.view_order == tc.view_order
    assert sorted(tc.view_order[-N_TRAIN:]) == list(range(N_TRAIN))            # the last epoch sees every view once
    assert set(vc) == {"loss", "psnr", "ssim", "inference_time", "loss_cc", "psnr_cc", "ssim_cc"} and set(vb) == set(va) == set(vc) - {"loss_cc", "psnr_cc", "ssim_cc"}
    A = tc.appearance_table.transforms.cpu().numpy().reshape(N_TRAIN, 3, 4)
    u, v = PAIR
    recovered, planted = A[v, 0, 0] / A[u, 0, 0], GAINS[v] / GAINS[u]
    print(f"last-epoch train/l1: plain {la:.5f}, altered {lb:.5f}, altered with the table {lc:.5f} (midpoint {(la + lb) / 2:.5f})")
    print(f"val/psnr: plain {va['psnr']:.3f}, altered {vb['psnr']:.3f}, altered with the table {vc['psnr']:.3f}; val/psnr_cc with the table {vc['psnr_cc']:.3f}")
    print(f"gain ratio of views {v} and {u}: recovered {recovered:.4f}, planted {planted:.4f}; the planted gains differ by {abs(GAINS[v] - GAINS[u]):.4f}")
    print("diagonal gains:", np.round(A[:, 0, 0], 4).tolist(), "offsets:", np.round(A[:, 0, 3], 4).tolist())
    assert lc < (la + lb) / 2
    assert vc["psnr_cc"] > vb["psnr"]
    assert abs(recovered - planted) < abs(GAINS[v] - GAINS[u])
    assert all(np.isfinite(x) for x in vc.values()) and 0 < vc["ssim_cc"] <= 1
    # the files of the validation: the table beside every scene
    model = tc.config.output_model_dir
    k = SCHEDULE["val_interval"]
    assert os.path.exists(os.path.join(model, f"scene_{k}.parquet")) and os.path.exists(os.path.join(model, f"appearance_{k}.pt"))
    assert os.path.exists(os.path.join(model, "best_scene.parquet")) and os.path.exists(os.path.join(model, "best_appearance.pt"))
    loaded, paths = AppearanceTable.load(os.path.join(model, f"appearance_{k}.pt"), DEV)
    assert torch.equal(loaded.transforms, tc.appearance_table.transforms) and loaded.steps == tc.appearance_table.steps
    assert paths == [r["image_path"] for r in json.load(open(data["altered"]["paths"]["train"]))]
    assert loaded.steps == [SCHEDULE["num_iterations"] // N_TRAIN] * N_TRAIN


def test_masks_and_the_fixed_budget_run_with_a_table(data, tmp_path):
    tables = {}
    for name in ("masked", "corrupted"):
        trainer = make_trainer(data[name], tmp_path / name, num_iterations=1, initial_downsample_factor=1, appearance="affine",
                               pixel_weights="file", mask_erode=5, log_loss_interval=1, log_metrics_interval=1, seed=3)
        trainer.train()
        means = trainer.validation(1)
        for t in (trainer.scene.point_cloud, trainer.scene.point_cloud_features, trainer.appearance_table.transforms,
                  trainer.appearance_table.exp_avg, trainer.appearance_table.exp_avg_sq):
            assert bool(torch.isfinite(t.detach()).all())
        assert all(np.isfinite(v) for v in means.values()) and "psnr_cc" in means
        tables[name] = trainer
    a, b = tables["masked"].appearance_table, tables["corrupted"].appearance_table
    assert not torch.equal(tables["masked"].train_targets.target(0, 1)[0], tables["corrupted"].train_targets.target(0, 1)[0])
    view = tables["masked"].view_order[0]
    assert bool(a.grad[view].any()) and a.steps[view] == 1
    # noise under the eroded mask: the loss's gradient is exactly 0 there, so those pixels are selected out of the table's sums
    for name in ("transforms", "grad", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    # the fixed-budget strategy beside the table
    config = TU.train_config(data["plain"]["paths"], tmp_path / "mcmc", num_iterations=1, initial_downsample_factor=2)
    config.gaussian_point_cloud_scene_config.max_num_points_ratio = 1.5
    trainer = GaussianPointCloudTrainer(config, device=DEV, writer=JsonlSummaryWriter(config.summary_writer_log_dir), density="mcmc",
                                        mcmc_config=MCMCConfig(cap_max=430, seed=3), appearance="affine")
    trainer.train()
    assert trainer.mcmc is not None and sum(trainer.appearance_table.steps) == 1
    for t in (trainer.scene.point_cloud, trainer.scene.point_cloud_features, trainer.appearance_table.transforms):
        assert bool(torch.isfinite(t.detach()).all())
    assert not torch.equal(trainer.appearance_table.transforms, AppearanceTable(N_TRAIN, DEV).transforms)


def _cli(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "gaussian_point_render.py"), "--device", DEV] + [str(a) for a in args], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return p


def test_render_script_corrects_exactly_the_frames_of_the_file(data, tmp_path):
    """two training views whose paths are in the table's file and two validation views whose paths are not"""
    train = json.load(open(data["plain"]["paths"]["train"]))[:2]
    val = json.load(open(data["plain"]["paths"]["val"]))
    poses = tmp_path / "four.json"
    poses.write_text(json.dumps(train + val))
    table = AppearanceTable(2, DEV)
    table.transforms[0] = torch.tensor([0.5, 0, 0, 0.1, 0, 0.5, 0, 0.1, 0, 0, 0.5, 0.1], device=DEV)
    table.transforms[1] = torch.tensor([0.8, 0.1, 0, 0, 0, 0.9, 0, 0, 0.1, 0, 0.7, 0.05], device=DEV)
    table.save(str(tmp_path / "appearance_7.pt"), [r["image_path"] for r in train])
    plain, corrected = tmp_path / "plain", tmp_path / "corrected"
    # without the flag: what the script does, in this process (tests/test_gpu_renderer.py runs it as a child)
    renderer = GaussianPointRenderer(GaussianPointRenderer.GaussianPointRendererConfig(data["plain"]["paths"]["cloud"], torch.eye(4).unsqueeze(0),
                                                                                       device=DEV), frame_format="png")
    os.makedirs(plain)
    without = renderer.run(plain, targets=TargetStore.from_dataset(ImagePoseDataset(dataset_json_path=str(poses)), device=DEV))
    _cli("--parquet_path", data["plain"]["paths"]["cloud"], "--poses", poses, "--output_prefix", corrected, "--appearance", tmp_path / "appearance_7.pt")
    frames = {d: [np.array(PIL.Image.open(d / f"frame_{i:03}.png")) for i in range(4)] for d in (plain, corrected)}
    for i in range(4):
        same = np.array_equal(frames[plain][i], frames[corrected][i])
        assert same == (i >= 2), i
    # frame 0 is the plain frame under 0.5 x + 0.1, up to the rounding of the two 8-bit conversions
    # (where the plain frame is not clamped)
    want = frames[plain][0].astype(np.float64) * 0.5 + 0.1 * 255.0
    inside = (frames[plain][0] > 0) & (frames[plain][0] < 255)
    assert inside.mean() > 0.1 and np.abs(frames[corrected][0].astype(np.float64) - want)[inside].max() <= 1.5
    with_ = json.loads((corrected / "metrics.json").read_text())
    assert set(without["mean"]) == {"psnr_8bit", "psnr", "ssim"} and all("psnr_cc" not in v for v in without["views"])
    assert set(with_["mean"]) == {"psnr_8bit", "psnr", "ssim", "psnr_cc"} and all(np.isfinite(v["psnr_cc"]) for v in with_["views"])
    for i in (2, 3):
        assert abs(with_["views"][i]["psnr"] - without["views"][i]["psnr"]) < 1e-4 and with_["views"][i]["sse_8bit"] == without["views"][i]["sse_8bit"]
        assert with_["views"][i]["psnr_cc"] >= with_["views"][i]["psnr"] - 1e-3        # the identity is among the affine maps
    for i in (0, 1):
        assert with_["views"][i]["psnr"] < without["views"][i]["psnr"]                 # a wrong transform makes the frame worse
        # both transforms are invertible and keep [0, 1] inside [0, 1]: the fit undoes them
        assert with_["views"][i]["psnr_cc"] > without["views"][i]["psnr"] - 0.5 and with_["views"][i]["psnr_cc"] > with_["views"][i]["psnr"]
