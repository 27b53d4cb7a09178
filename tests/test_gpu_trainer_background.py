"""GPU (-m gpu): backgrounds through GaussianPointCloudTrainer(config, background=...) on the 64x96 views of
tests/trainer_util.py's dataset: "none" is the loop as it was, the constructor refuses what cannot work, the first "sky"
iteration is the step written out by hand, a sky trained on pictures with a planted sky behind the scene takes it up, RGBA
pictures are composited over the step's colour, and the render script composites over a colour or over the file the trainer
wrote."""
import json
import os
import subprocess
import sys

import numpy as np
import PIL.Image
import pytest
import torch

import background_ref as ref
import trainer_util as TU
from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast, background
from taichi_3d_gaussian_splatting_amd.appearance import AppearanceTable
from taichi_3d_gaussian_splatting_amd.background import BackgroundConfig, BackgroundModel
from taichi_3d_gaussian_splatting_amd.GaussianPointAdaptiveController import GaussianPointAdaptiveController
from taichi_3d_gaussian_splatting_amd.GaussianPointCloudScene import GaussianPointCloudScene
from taichi_3d_gaussian_splatting_amd.GaussianPointRenderer import GaussianPointRenderer
from taichi_3d_gaussian_splatting_amd.GaussianPointTrainer import GaussianPointCloudTrainer, JsonlSummaryWriter
from taichi_3d_gaussian_splatting_amd.ImagePoseDataset import ImagePoseDataset
from taichi_3d_gaussian_splatting_amd.LossFunction import LossFunction
from taichi_3d_gaussian_splatting_amd.mcmc import MCMCConfig
from taichi_3d_gaussian_splatting_amd.optim import FusedAdam
from taichi_3d_gaussian_splatting_amd.synthetic import scene_input, view_pose
from taichi_3d_gaussian_splatting_amd.targets import TargetStore
from test_gpu_trainer import hand_written_loop

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_TRAIN = len(TU.TRAIN_VIEWS)
N_VIEWS = len(TU.TRAIN_VIEWS) + len(TU.VAL_VIEWS)
SCHEDULE = dict(TU.SMOKE)           # 120 iterations: 20 steps per view
# The planted sky: band 1, a vertical gradient in the scene's frame (Y_1 = -0.4886 d_y, and y points down in the pictures), the
# same slope in every channel.  |Y_1| < 0.49, so a channel stays within its constant -+ 0.1: between 0.25 and 0.75, and a
# premultiplied colour x <= A leaves x + (1 - A) c below 1.  The dataset fixture asserts that nothing saturates.
PLANTED_CONSTANT = (0.35, 0.5, 0.65)
PLANTED_SLOPE = 0.2
SKY = dict(colour=(0.5, 0.5, 0.5), bands=1)            # the model of run (c): starts as a mid grey, default learning rates


def planted_coefficients():
    coef = np.zeros((3, 16), dtype=np.float32)
    coef[:, 0], coef[:, 1] = PLANTED_CONSTANT, PLANTED_SLOPE
    return coef.reshape(48)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """trainer_util's dataset from the perturbed scene: `plain`; `planted`: every training and validation picture with the
    planted sky behind the ground-truth scene; `rgba`: the plain pictures with the rendered accumulated alpha as channel 3"""
    root = tmp_path_factory.mktemp("background_data")
    base = TU.write_dataset(root, DEV, initial=TU.perturbed(TU.ground_truth_scene()))
    records = {split: json.load(open(base["paths"][split])) for split in ("train", "val")}
    out = {"plain": base, "coverage": []}
    scene = TU.ground_truth_scene()
    module = Rast(Rast.GaussianPointCloudRasterisationConfig())
    coef = planted_coefficients()
    os.makedirs(root / "planted", exist_ok=True)
    os.makedirs(root / "rgba", exist_ok=True)
    by_view = {}
    with torch.no_grad():
        for view in range(N_VIEWS):
            q, t = view_pose(view, N_VIEWS)
            image, _, _, alpha = module(scene_input(scene, q, t, DEV, band=3), return_accumulated_alpha=True)
            x, A = image.permute(2, 0, 1).contiguous().cpu().numpy(), alpha.cpu().numpy()
            assert np.array_equal((image.clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy(), base["images"][view])
            over = ref.composite(x, A, coef, 1, q[0], scene.camera_intrinsics)
            assert over.min() >= 0.0 and over.max() < 1.0, "a channel would saturate"
            sky = ref.colours(coef, 1, q[0], scene.camera_intrinsics, TU.H, TU.W)
            assert sky.min() > 0.2 and sky.max() < 0.8
            PIL.Image.fromarray(np.round(over.transpose(1, 2, 0) * 255).astype(np.uint8)).save(root / "planted" / f"view_{view}.png")
            rgba = np.concatenate([base["images"][view], np.round(np.clip(A, 0, 1) * 255).astype(np.uint8)[:, :, None]], axis=2)
            PIL.Image.fromarray(rgba, mode="RGBA").save(root / "rgba" / f"view_{view}.png")
            by_view[view] = A
            out["coverage"].append(float((A < 0.5).mean()))
    assert min(out["coverage"]) > 0.05, "the background must show in every view"

    def variant(name):
        paths = dict(base["paths"], train=str(root / f"train_{name}.json"), val=str(root / f"val_{name}.json"))
        for split in ("train", "val"):
            moved = [dict(r, image_path=str(root / name / os.path.basename(r["image_path"]))) for r in records[split]]
            json.dump(moved, open(paths[split], "w"))
        out[name] = dict(paths=paths, images=base["images"])

    variant("planted")
    variant("rgba")
    out["alpha"] = by_view
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
    trainer = make_trainer(data["plain"], tmp_path, num_iterations=n_it, initial_downsample_factor=1, background="none",
                           increase_color_max_sh_band_interval=band_interval, position_learning_rate_decay_interval=decay_interval,
                           position_learning_rate_decay_rate=rate, position_learning_rate=1e-4, seed=3)
    assert trainer.background == "none" and trainer.background_model is None and trainer.composite_targets is False
    trainer.train()
    scene, _, _ = hand_written_loop(data["plain"], trainer.config, trainer.view_order, n_it, band_interval, decay_interval, rate, False, seed=3)
    assert torch.equal(trainer.scene.point_cloud, scene.point_cloud)
    assert torch.equal(trainer.scene.point_cloud_features, scene.point_cloud_features)
    means = trainer.validation(n_it)
    assert set(means) == {"loss", "psnr", "ssim", "inference_time"}
    assert not any("background" in f for f in os.listdir(trainer.config.output_model_dir))
    assert not hasattr(GaussianPointCloudTrainer.TrainConfig(), "background")


def test_the_constructor_refuses_what_cannot_work(data, tmp_path):
    for i, (match, kwargs) in enumerate([
            ("background must be", dict(background="white")),
            ("need a background", dict(background_config=BackgroundConfig())),
            ("need a background", dict(composite_targets=True)),
            ("composite_targets=True", dict(background="random")),
            ('pixel_weights="file"', dict(background="colour", composite_targets=True, pixel_weights="file")),
            ("rgb_only", dict(background="sky", rgb_only=True)),
            ("targets_on_device", dict(background="sky", targets_on_device=False)),
            ("bands", dict(background="sky", background_config=BackgroundConfig(bands=5))),
            ("no alpha channel", dict(background="colour", composite_targets=True))]):            # the plain pictures are RGB
        rgb_only = kwargs.pop("rgb_only", False)
        fields = {f for f in GaussianPointCloudTrainer.TrainConfig.__dataclass_fields__}
        config = TU.train_config(data["plain"]["paths"], tmp_path / str(i), **{k: v for k, v in kwargs.items() if k in fields})
        config.rasterisation_config.rgb_only = rgb_only
        with pytest.raises(ValueError, match=match):
            GaussianPointCloudTrainer(config, device=DEV, writer=JsonlSummaryWriter(config.summary_writer_log_dir),
                                      **{k: v for k, v in kwargs.items() if k not in fields})


def test_first_sky_iteration_is_the_manual_step(data, tmp_path):
    factor = 2
    sky = BackgroundConfig(colour=(0.3, 0.4, 0.5), bands=2)
    trainer = make_trainer(data["planted"], tmp_path, num_iterations=1, initial_downsample_factor=factor, background="sky",
                           background_config=sky, log_loss_interval=1, log_metrics_interval=10 ** 6, position_learning_rate=1e-4, seed=3)
    model = trainer.background_model
    assert (model.kind, model.bands, model.config.num_iterations) == ("sky", 2, 1) and (model.config.lr, model.config.lr_final) == (0.01, 0.001)
    trainer.train()
    torch.cuda.synchronize()
    view = trainer.view_order[0]

    config = trainer.config
    scene = GaussianPointCloudScene.from_parquet(data["planted"]["paths"]["cloud"], config=config.gaussian_point_cloud_scene_config, device=DEV)
    controller = GaussianPointAdaptiveController(
        config=config.adaptive_controller_config,
        maintained_parameters=GaussianPointAdaptiveController.GaussianPointAdaptiveControllerMaintainedParameters(
            pointcloud=scene.point_cloud, pointcloud_features=scene.point_cloud_features,
            point_invalid_mask=scene.point_invalid_mask, point_object_id=scene.point_object_id), seed=3)
    rast = Rast(Rast.GaussianPointCloudRasterisationConfig(), backward_valid_point_hook=controller.update)
    loss_fn = LossFunction(LossFunction.LossFunctionConfig())
    of = FusedAdam([scene.point_cloud_features], lr=config.feature_learning_rate)
    op = FusedAdam([scene.point_cloud], lr=config.position_learning_rate)
    manual = BackgroundModel("sky", DEV, BackgroundConfig(colour=(0.3, 0.4, 0.5), bands=2, num_iterations=1))
    gt, q, t, info = TargetStore.from_dataset(ImagePoseDataset(data["planted"]["paths"]["train"]), DEV).target(view, factor)
    img, _, _, alpha = rast(Rast.GaussianPointCloudRasterisationInput(
        point_cloud=scene.point_cloud, point_cloud_features=scene.point_cloud_features, point_object_id=scene.point_object_id,
        point_invalid_mask=scene.point_invalid_mask, camera_info=info, q_pointcloud_camera=q, t_pointcloud_camera=t,
        color_max_sh_band=0), return_accumulated_alpha=True)
    composited = background.composite(img.permute(2, 0, 1), alpha, manual.coef_for_step(), 2, q, info.camera_intrinsics)
    L, l1, ld = loss_fn(composited, gt, point_invalid_mask=scene.point_invalid_mask, pointcloud_features=scene.point_cloud_features,
                        clamp_predicted=True)
    L.backward()
    of.step(); op.step(); manual.step(0)
    controller.refinement()
    torch.cuda.synchronize()
    assert logged(trainer, "train/loss") == [(0, float(L.item()))] and logged(trainer, "train/l1 loss") == [(0, float(l1.item()))]
    assert torch.equal(trainer.scene.point_cloud, scene.point_cloud) and torch.equal(trainer.scene.point_cloud_features, scene.point_cloud_features)
    for name in ("coef", "grad", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(model, name), getattr(manual, name)), name
    assert model.steps == manual.steps == 1
    moved = (model.coef != background.colour_coefficients((0.3, 0.4, 0.5), DEV)).cpu().numpy().reshape(3, 16)
    assert moved[:, :9].all() and not moved[:, 9:].any() and bool(model.grad.view(3, 16)[:, :9].all())


def test_a_trained_sky_takes_up_a_planted_one(data, tmp_path):
    """Three runs of trainer_util.SMOKE (120 iterations, 20 per view), the same initial scene and seed: (a) plain pictures
    without a model, (b) pictures with the planted sky without a model -- the code as it was -- and (c) the same pictures with
    background="sky".  Asserted: the stronger bar of the appearance test, last-epoch L1 of (c) below the midpoint of (a) and
    (b) -- which implies the required (c) below (b) -- and val/psnr of (c) above that of (b).

    Measured on an MI355X (profiles/background_margins.json): the background shows in 77 .. 80 % of a picture; last-epoch
    train/l1 0.00596 (a), 0.12265 (b), 0.00379 (c), midpoint 0.06431; val/psnr 39.03 (a), 16.35 (b), 44.55 dB (c).  Recovered
    slopes on Y_1 0.203 / 0.199 / 0.197 for a planted 0.2; the constants 0.393 / 0.500 / 0.607 for 0.35 / 0.5 / 0.65 come with
    -0.099 / 0.000 / +0.099 on Y_2: every camera of the dataset looks along +z of the scene, where Y_2 is about 0.45 in every
    pixel, so the constant and Y_2 are told apart only weakly and Adam moves both by the same amount (0.393 - 0.099 * 0.45 = 0.35)."""
    runs = {}
    for name, images, kwargs in (("a", "plain", {}), ("b", "planted", {}),
                                 ("c", "planted", dict(background="sky", background_config=BackgroundConfig(**SKY)))):
        trainer = make_trainer(data[images], tmp_path / name, regularise=False, log_loss_interval=1, log_metrics_interval=10 ** 6, seed=0,
                               **SCHEDULE, **kwargs)
        trainer.train()
        iteration, means = trainer.last_validation
        assert iteration == SCHEDULE["val_interval"]
        l1 = logged(trainer, "train/l1 loss")
        assert [s for s, _ in l1] == list(range(SCHEDULE["num_iterations"]))
        runs[name] = (trainer, means, float(np.mean([v for _, v in l1[-N_TRAIN:]])))
    (ta, va, la), (tb, vb, lb), (tc, vc, lc) = runs["a"], runs["b"], runs["c"]
    assert ta.view_order == tb.view_order == tc.view_order
    assert sorted(tc.view_order[-N_TRAIN:]) == list(range(N_TRAIN))            # the last epoch sees every view once
    assert set(va) == set(vb) == set(vc) == {"loss", "psnr", "ssim", "inference_time"}         # the metric names are unchanged
    recovered = tc.background_model.coef.cpu().numpy().reshape(3, 16)
    print(f"background visible (alpha < 0.5) in {min(data['coverage']):.2f} .. {max(data['coverage']):.2f} of a picture")
    print(f"last-epoch train/l1: plain {la:.5f}, planted {lb:.5f}, planted with the sky {lc:.5f} (midpoint {(la + lb) / 2:.5f})")
    print(f"val/psnr: plain {va['psnr']:.3f}, planted {vb['psnr']:.3f}, planted with the sky {vc['psnr']:.3f}")
    print("recovered constants", np.round(recovered[:, 0], 4).tolist(), "planted", list(PLANTED_CONSTANT))
    print("recovered band 1 (Y_1, Y_2, Y_3)", np.round(recovered[:, 1:4], 4).tolist(), "planted", [PLANTED_SLOPE, 0.0, 0.0])
    assert lc < (la + lb) / 2 and lb > la                                      # the stronger bar: below the midpoint, so below (b)
    assert vc["psnr"] > vb["psnr"]
    assert all(np.isfinite(x) for x in vc.values()) and bool(torch.isfinite(tc.background_model.coef).all())
    assert not recovered[:, 4:].any()                                          # one band: the others stay where they were
    # the files of the validation: the background beside every scene
    model = tc.config.output_model_dir
    k = SCHEDULE["val_interval"]
    assert os.path.exists(os.path.join(model, f"scene_{k}.parquet")) and os.path.exists(os.path.join(model, f"background_{k}.pt"))
    assert os.path.exists(os.path.join(model, "best_scene.parquet")) and os.path.exists(os.path.join(model, "best_background.pt"))
    loaded = BackgroundModel.load(os.path.join(model, f"background_{k}.pt"), DEV)
    assert (loaded.kind, loaded.bands, loaded.steps) == ("sky", 1, SCHEDULE["num_iterations"])
    assert torch.equal(loaded.coef, tc.background_model.coef)
    assert not any("background" in f for f in os.listdir(tb.config.output_model_dir))


class _TargetRecorder:
    """the trainer's loss function, keeping a copy of every target it is given"""

    def __init__(self, inner):
        self.inner, self.targets = inner, []

    def __call__(self, image_pred, image_gt, **kwargs):
        self.targets.append((image_gt.clone(), None if kwargs.get("pixel_weight") is None else kwargs["pixel_weight"].clone()))
        return self.inner(image_pred, image_gt, **kwargs)


@pytest.mark.parametrize("kind", ["colour", "random"])
def test_rgba_pictures_are_composited_over_the_steps_colour(data, tmp_path, kind):
    factor = 2
    cfg = BackgroundConfig(colour=(1.0, 1.0, 1.0), seed=5)
    trainer = make_trainer(data["rgba"], tmp_path, num_iterations=1, initial_downsample_factor=factor, background=kind,
                           background_config=cfg, composite_targets=True, log_loss_interval=1, log_metrics_interval=1, seed=3)
    assert trainer.weighted is False and trainer.background_model.bands == 0
    recorder = trainer.loss_function = _TargetRecorder(trainer.loss_function)
    trainer.train()
    for t in (trainer.scene.point_cloud, trainer.scene.point_cloud_features):
        assert bool(torch.isfinite(t.detach()).all())
    target, weight = recorder.targets[0]
    assert weight is None                                           # the alpha is no weight unless one is asked for
    view = trainer.view_order[0]
    store = TargetStore.from_dataset(ImagePoseDataset(data["rgba"]["paths"]["train"]), DEV, mask_source="alpha")
    rgb, q, t, info, alpha = store.target(view, factor, with_weight=True)
    coef = BackgroundModel(kind, DEV, BackgroundConfig(colour=(1.0, 1.0, 1.0), seed=5)).coef_for_step()
    want = background.composite_straight(torch.cat([rgb, alpha[None]]), coef, 0)
    assert torch.equal(target, want)
    colour = coef.view(3, 16)[:, 0]
    assert bool((colour == 1.0).all()) == (kind == "colour")
    assert torch.equal(want, rgb * alpha + (1.0 - alpha) * colour[:, None, None])
    # validation composites rendering and pictures over the stored colour: white, for "random" too
    means = trainer.validation(1)
    assert all(np.isfinite(v) for v in means.values())
    assert bool((trainer.background_model.coef.view(3, 16)[:, 0] == 1.0).all())
    val_store = TargetStore.from_dataset(ImagePoseDataset(data["rgba"]["paths"]["val"]), DEV, mask_source="alpha")
    rgb, _, _, _, alpha = val_store.target(len(TU.VAL_VIEWS) - 1, 1, with_weight=True)
    assert torch.equal(recorder.targets[-1][0], rgb * alpha + (1.0 - alpha))


def test_backgrounds_combine_with_weights_a_table_and_the_fixed_budget(data, tmp_path):
    # the alpha as the loss's weight beside the compositing
    trainer = make_trainer(data["rgba"], tmp_path / "weights", num_iterations=1, initial_downsample_factor=2, background="random",
                           composite_targets=True, pixel_weights="alpha", seed=3)
    recorder = trainer.loss_function = _TargetRecorder(trainer.loss_function)
    trainer.train()
    assert trainer.weighted and recorder.targets[0][1] is not None and recorder.targets[0][1].shape == recorder.targets[0][0].shape[1:]
    # an appearance table behind the compositing
    trainer = make_trainer(data["rgba"], tmp_path / "affine", num_iterations=1, initial_downsample_factor=2, background="colour",
                           background_config=BackgroundConfig(colour=(1.0, 1.0, 1.0)), composite_targets=True, appearance="affine", seed=3)
    trainer.train()
    assert sum(trainer.appearance_table.steps) == 1
    assert not torch.equal(trainer.appearance_table.transforms, AppearanceTable(N_TRAIN, DEV).transforms)
    for t in (trainer.scene.point_cloud, trainer.scene.point_cloud_features, trainer.appearance_table.transforms):
        assert bool(torch.isfinite(t.detach()).all())
    means = trainer.validation(1)
    assert "psnr_cc" in means and all(np.isfinite(v) for v in means.values())
    # the fixed-budget strategy beside a sky and beside a random colour
    for name, kwargs in (("sky", dict(background="sky")), ("random", dict(background="random", composite_targets=True))):
        config = TU.train_config(data["rgba" if name == "random" else "planted"]["paths"], tmp_path / f"mcmc_{name}", num_iterations=1,
                                 initial_downsample_factor=2)
        config.gaussian_point_cloud_scene_config.max_num_points_ratio = 1.5
        trainer = GaussianPointCloudTrainer(config, device=DEV, writer=JsonlSummaryWriter(config.summary_writer_log_dir), density="mcmc",
                                            mcmc_config=MCMCConfig(cap_max=430, seed=3), **kwargs)
        trainer.train()
        assert trainer.mcmc is not None and trainer.background_model.steps == (1 if name == "sky" else 0)
        for t in (trainer.scene.point_cloud, trainer.scene.point_cloud_features, trainer.background_model.coef):
            assert bool(torch.isfinite(t.detach()).all())


def _cli(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "gaussian_point_render.py"), "--device", DEV] + [str(a) for a in args], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return p


def test_render_script_composites_over_a_colour_and_over_a_saved_sky(data, tmp_path):
    cloud = data["plain"]["paths"]["cloud"]
    poses = torch.stack([torch.tensor(json.load(open(data["plain"]["paths"]["val"]))[i]["T_pointcloud_camera"], dtype=torch.float32) for i in range(2)])
    torch.save(poses, tmp_path / "poses.pt")
    K = TU.ground_truth_scene().camera_intrinsics
    size = ["--image_height", TU.H, "--image_width", TU.W, "--camera_intrinsics", K[0, 0], K[1, 1], K[0, 2], K[1, 2]]
    sky = BackgroundModel("sky", DEV, BackgroundConfig(colour=PLANTED_CONSTANT, bands=1))
    sky.coef.copy_(torch.tensor(planted_coefficients(), device=DEV))
    sky.save(str(tmp_path / "background_7.pt"))
    plain, white, saved, here = (tmp_path / name for name in ("plain", "white", "saved", "here"))
    _cli("--parquet_path", cloud, "--poses", tmp_path / "poses.pt", "--output_prefix", white, "--background", "white", *size)
    _cli("--parquet_path", cloud, "--poses", tmp_path / "poses.pt", "--output_prefix", saved, "--background", tmp_path / "background_7.pt", *size)
    # what the script does without the flag, and with the model given directly, in this process
    config = GaussianPointRenderer.GaussianPointRendererConfig(cloud, poses, device=DEV, image_height=TU.H, image_width=TU.W,
                                                               camera_intrinsics=torch.tensor(K))
    renderer = GaussianPointRenderer(config, frame_format="png")
    for d in (plain, here):
        os.makedirs(d)
    renderer.run(plain)
    renderer.run(here, background=BackgroundModel.load(str(tmp_path / "background_7.pt"), DEV))
    q_rows, t_rows = renderer.pose_rows()
    for i in range(2):
        frames = {d: np.array(PIL.Image.open(d / f"frame_{i:03}.png")) for d in (plain, white, saved, here)}
        image, _, alpha = renderer.render(q_rows[i], t_rows[i], alpha=True)
        alpha = alpha.cpu().numpy()
        empty, full = alpha == 0.0, alpha == 1.0
        assert empty.mean() > 0.02, "no pixel without a splat"
        assert np.all(frames[white][empty] == 255)
        assert np.array_equal(frames[white][full], frames[plain][full])
        print(f"frame {i}: {empty.mean():.3f} of the pixels have alpha 0, {full.mean():.3f} alpha 1")
        # every pixel: the plain frame under x + (1 - A), to the rounding of the 8-bit conversion
        want = np.clip(image.cpu().numpy() + (1.0 - alpha)[:, :, None], 0.0, 1.0) * 255.0
        assert np.abs(frames[white][...].astype(np.float64) - want).max() <= 1.0
        assert np.array_equal(frames[saved], frames[here]) and not np.array_equal(frames[saved], frames[plain])
        over = ref.composite(image.permute(2, 0, 1).cpu().numpy(), alpha, planted_coefficients(), 1, q_rows[i, 0].cpu().numpy(), K)
        assert np.abs(frames[saved].astype(np.float64) - np.clip(over.transpose(1, 2, 0), 0.0, 1.0) * 255.0).max() <= 1.0
