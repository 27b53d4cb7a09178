"""GPU (-m gpu): the 3D smoothing filter through GaussianPointCloudTrainer(config, filter3d=...): None is the loop as it was,
the rates follow a refinement that adds rows, the table files are written beside the scene and load back, and the protocol of
the Mip-Splatting paper in small: trained at a quarter of the pictures' resolution, validated at the full one, with and
without the filter.  GS_FILTER3D_MARGINS_OUT=<file> records the protocol run's numbers (profiles/filter3d_margins.json holds a
run)."""
import json
import os

import numpy as np
import PIL.Image
import pytest
import torch

import trainer_util as TU
from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast, filter3d, scene_io
from taichi_3d_gaussian_splatting_amd.Camera import CameraInfo
from taichi_3d_gaussian_splatting_amd.filter3d import Filter3D, Filter3DConfig
from taichi_3d_gaussian_splatting_amd.GaussianPointCloudScene import GaussianPointCloudScene
from taichi_3d_gaussian_splatting_amd.GaussianPointTrainer import GaussianPointCloudTrainer, JsonlSummaryWriter
from taichi_3d_gaussian_splatting_amd.synthetic import view_pose
from taichi_3d_gaussian_splatting_amd.utils import quaternion_to_rotation_matrix_torch
from test_gpu_trainer import hand_written_loop

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_VIEWS = len(TU.TRAIN_VIEWS) + len(TU.VAL_VIEWS)
SCALE = 4                                                   # the protocol's pictures: 256 x 384
# trained at a fixed factor 4 (the 64x96 frames of every other trainer test) for the suite's usual 120 iterations, validated at
# iteration 119 at factor 1
PROTOCOL = dict(TU.SMOKE, initial_downsample_factor=SCALE, half_downsample_factor_interval=10 ** 6)
# What the protocol measured on an MI355X (profiles/filter3d_margins.json): val/psnr at factor 1 and at factor 4, without and
# with the filter.  The assertion of test_trained_at_a_quarter_validated_at_full_resolution is taken from these: the filter
# does not raise the factor-1 PSNR of this run, so what is asserted is that the factor-4 PSNR with the filter stays within the
# measured gap of the run without it, 3.627 dB, with a tenth of it for another build or device.
MEASURED = dict(val_psnr_factor_1=dict(plain=34.537, filter=30.914), val_psnr_factor_4=dict(plain=37.419, filter=33.792))
SEPARATES = MEASURED["val_psnr_factor_1"]["filter"] > MEASURED["val_psnr_factor_1"]["plain"]
GAP_DB = 1.1 * (MEASURED["val_psnr_factor_4"]["plain"] - MEASURED["val_psnr_factor_4"]["filter"])


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    return TU.write_dataset(tmp_path_factory.mktemp("filter3d_data"), DEV, initial=TU.perturbed(TU.ground_truth_scene()))


def write_large_dataset(root):
    """trainer_util's scene and views with the pictures rendered at SCALE times the size: every intrinsic times SCALE (pixel
    centres are at +0.5, so the frames are the same frames, sampled finer).  -> the paths"""
    root = str(root)
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    scene = TU.ground_truth_scene()
    K = scene.camera_intrinsics.copy()
    K[:2, :] *= SCALE
    height, width = TU.H * SCALE, TU.W * SCALE
    module = Rast(Rast.GaussianPointCloudRasterisationConfig())
    dev = lambda a: torch.tensor(a, device=DEV)
    records = {}
    with torch.no_grad():
        for view in range(N_VIEWS):
            q, t = view_pose(view, N_VIEWS)
            image = module(Rast.GaussianPointCloudRasterisationInput(
                point_cloud=dev(scene.point_cloud), point_cloud_features=dev(scene.point_cloud_features), point_object_id=dev(scene.point_object_id),
                point_invalid_mask=dev(scene.point_invalid_mask), camera_info=CameraInfo(dev(K), height, width, 0),
                q_pointcloud_camera=dev(q), t_pointcloud_camera=dev(t), color_max_sh_band=3))[0]
            path = os.path.join(root, "images", f"view_{view}.png")
            PIL.Image.fromarray((image.clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy()).save(path)
            T = np.eye(4)
            T[:3, :3] = quaternion_to_rotation_matrix_torch(torch.tensor(q, dtype=torch.float64))[0].numpy()
            T[:3, 3] = t[0]
            records[view] = dict(image_path=path, T_pointcloud_camera=T.tolist(), camera_intrinsics=K.tolist(), camera_height=height,
                                 camera_width=width, camera_id=0)
    paths = dict(train=os.path.join(root, "train.json"), val=os.path.join(root, "val.json"), cloud=os.path.join(root, "point_cloud.parquet"))
    for name, views in (("train", TU.TRAIN_VIEWS), ("val", TU.VAL_VIEWS)):
        with open(paths[name], "w") as fh:
            json.dump([records[v] for v in views], fh)
    scene_io.save_parquet(paths["cloud"], *TU.perturbed(scene))
    return paths


def make_trainer(paths, out_dir, regularise=True, densify=False, **kwargs):
    """kwargs that TrainConfig has are config overrides, the others constructor arguments"""
    fields = {f for f in GaussianPointCloudTrainer.TrainConfig.__dataclass_fields__}
    config = TU.train_config(paths, out_dir, densify=densify, **{k: v for k, v in kwargs.items() if k in fields})
    config.loss_function_config.enable_regularization = regularise
    return GaussianPointCloudTrainer(config, device=DEV, writer=JsonlSummaryWriter(config.summary_writer_log_dir),
                                     **{k: v for k, v in kwargs.items() if k not in fields})


def test_none_is_the_loop_as_it_was(data, tmp_path):
    n_it, band_interval, decay_interval, rate = 3, 2, 2, 0.9
    trainer = make_trainer(data["paths"], tmp_path, num_iterations=n_it, initial_downsample_factor=1, filter3d=None,
                           increase_color_max_sh_band_interval=band_interval, position_learning_rate_decay_interval=decay_interval,
                           position_learning_rate_decay_rate=rate, position_learning_rate=1e-4, seed=3)
    assert trainer.filter3d is None
    trainer.train()
    scene, _, _ = hand_written_loop(data, trainer.config, trainer.view_order, n_it, band_interval, decay_interval, rate, False, seed=3)
    assert torch.equal(trainer.scene.point_cloud, scene.point_cloud)
    assert torch.equal(trainer.scene.point_cloud_features, scene.point_cloud_features)
    means = trainer.validation(n_it)
    assert set(means) == {"loss", "psnr", "ssim", "inference_time"}
    assert not any("filter3d" in f for f in os.listdir(trainer.config.output_model_dir))


def test_the_first_filtered_iteration_is_the_manual_step(data, tmp_path):
    """one iteration at factor 2 with the filter against the same step written out: the view table of the dataset, the rates,
    the apply node in front of the rasteriser, the raw parameters under the regulariser and Adam"""
    from taichi_3d_gaussian_splatting_amd.GaussianPointAdaptiveController import GaussianPointAdaptiveController
    from taichi_3d_gaussian_splatting_amd.ImagePoseDataset import ImagePoseDataset
    from taichi_3d_gaussian_splatting_amd.LossFunction import LossFunction
    from taichi_3d_gaussian_splatting_amd.optim import FusedAdam
    from taichi_3d_gaussian_splatting_amd.targets import TargetStore
    factor = 2
    trainer = make_trainer(data["paths"], tmp_path, num_iterations=1, initial_downsample_factor=factor, filter3d=Filter3DConfig(),
                           log_loss_interval=1, log_metrics_interval=10 ** 6, position_learning_rate=1e-4, seed=3)
    assert trainer.filter3d.near == 0.8 and (trainer.filter3d.width, trainer.filter3d.height) == (TU.W, TU.H)
    assert trainer.filter3d.views.shape == (len(TU.TRAIN_VIEWS), 16)
    trainer.train()
    view = trainer.view_order[0]
    config = trainer.config
    scene = GaussianPointCloudScene.from_parquet(data["paths"]["cloud"], config=config.gaussian_point_cloud_scene_config, device=DEV)
    controller = GaussianPointAdaptiveController(
        config=config.adaptive_controller_config,
        maintained_parameters=GaussianPointAdaptiveController.GaussianPointAdaptiveControllerMaintainedParameters(
            pointcloud=scene.point_cloud, pointcloud_features=scene.point_cloud_features,
            point_invalid_mask=scene.point_invalid_mask, point_object_id=scene.point_object_id), seed=3)
    rast = Rast(Rast.GaussianPointCloudRasterisationConfig(), backward_valid_point_hook=controller.update)
    loss_fn = LossFunction(LossFunction.LossFunctionConfig())
    of = FusedAdam([scene.point_cloud_features], lr=config.feature_learning_rate)
    op = FusedAdam([scene.point_cloud], lr=config.position_learning_rate)
    dataset = ImagePoseDataset(data["paths"]["train"])
    rate = filter3d.sampling_rate(scene.point_cloud.detach(), scene.point_invalid_mask, filter3d.view_table(dataset, device=DEV), TU.W, TU.H)
    gt, q, t, info = TargetStore.from_dataset(dataset, DEV).target(view, factor)
    features = filter3d.apply(scene.point_cloud_features, rate, filter3d.filter_k(0.2, factor))
    img, _, _ = rast(Rast.GaussianPointCloudRasterisationInput(
        point_cloud=scene.point_cloud, point_cloud_features=features, point_object_id=scene.point_object_id,
        point_invalid_mask=scene.point_invalid_mask, camera_info=info, q_pointcloud_camera=q, t_pointcloud_camera=t, color_max_sh_band=0))
    L = loss_fn(img.permute(2, 0, 1), gt, point_invalid_mask=scene.point_invalid_mask, pointcloud_features=scene.point_cloud_features,
                clamp_predicted=True)[0]
    L.backward()
    of.step(); op.step()
    controller.refinement()
    torch.cuda.synchronize()
    assert torch.equal(trainer.scene.point_cloud, scene.point_cloud) and torch.equal(trainer.scene.point_cloud_features, scene.point_cloud_features)
    assert torch.equal(trainer.filter3d.rate.view(torch.int32), rate.view(torch.int32)) and trainer.filter3d.refreshes == 2
    # the filter was in the step: without it the same iteration ends elsewhere
    plain = make_trainer(data["paths"], tmp_path / "plain", num_iterations=1, initial_downsample_factor=factor, log_loss_interval=1,
                         log_metrics_interval=10 ** 6, position_learning_rate=1e-4, seed=3)
    plain.train()
    assert not torch.equal(plain.scene.point_cloud_features, trainer.scene.point_cloud_features)


def test_rates_follow_a_refinement_that_adds_rows(data, tmp_path):
    """trainer_util's densifying run (a cycle at iterations 2, 4 and 6) stopped behind iteration 6: the last thing that touched
    the scene is a refinement, so the buffer must hold the rates of the scene as it stands"""
    trainer = make_trainer(data["paths"], tmp_path, densify=True, num_iterations=7, initial_downsample_factor=2, position_learning_rate=1e-4,
                           seed=3, filter3d=Filter3DConfig(interval=10 ** 6))
    filt = trainer.filter3d
    valid_before = trainer.scene.point_invalid_mask == 0
    assert filt.refreshes == 1 and bool(torch.isinf(filt.rate[~valid_before]).all()) and bool(torch.isfinite(filt.rate[valid_before]).all())
    trainer.train()
    calls = trainer.adaptive_controller.refinement_calls
    assert calls == 3 and filt.refreshes == 2 + calls          # the constructor, iteration 0 and every refinement; no interval fell in the run
    valid = trainer.scene.point_invalid_mask == 0
    added = valid & ~valid_before
    print(f"valid rows {int(valid_before.sum())} -> {int(valid.sum())}, {int(added.sum())} of them in rows that were free")
    assert int(added.sum()) > 50
    rate = filt.rate
    assert bool(torch.isfinite(rate[valid]).all()) and bool((rate[valid] > 0).all()), "a new row kept the +inf of a free row"
    assert bool(torch.isinf(rate[~valid]).all())
    want = filter3d.sampling_rate(trainer.scene.point_cloud.detach(), trainer.scene.point_invalid_mask, filt.views, TU.W, TU.H, 0.8, 0.15)
    assert torch.equal(rate.view(torch.int32), want.view(torch.int32))
    # the fixed-budget strategy changes rows too
    from taichi_3d_gaussian_splatting_amd.mcmc import MCMCConfig
    config = TU.train_config(data["paths"], tmp_path / "mcmc", num_iterations=5, initial_downsample_factor=2)
    config.gaussian_point_cloud_scene_config.max_num_points_ratio = 1.5
    mcmc = GaussianPointCloudTrainer(config, device=DEV, writer=JsonlSummaryWriter(config.summary_writer_log_dir), density="mcmc",
                                     mcmc_config=MCMCConfig(cap_max=430, seed=3, refine_start=1, refine_every=2, refine_stop=100),
                                     filter3d=Filter3DConfig(interval=10 ** 6))
    mcmc.train()
    assert mcmc.mcmc.refinement_calls == 2 and mcmc.filter3d.refreshes == 2 + 2
    valid = mcmc.scene.point_invalid_mask == 0
    assert bool(torch.isfinite(mcmc.filter3d.rate[valid]).all()) and bool(torch.isinf(mcmc.filter3d.rate[~valid]).all())


def psnr_at(trainer, factor):
    """the mean PSNR of the validation views at a downsample factor, as validation() measures it at factor 1"""
    total = 0.0
    with torch.no_grad():
        for view in range(len(trainer.val_dataset)):
            image_gt, q, t, info = trainer.val_targets.target(view, factor)
            image = trainer.rasterisation(trainer._rasterisation_input(info, q, t, color_max_sh_band=3, downsample_factor=factor))[0]
            total += trainer._metrics(torch.clamp(image, 0, 1).permute(2, 0, 1), image_gt)[1].item()
    return total / len(trainer.val_dataset)


def protocol(root):
    """-> ({"plain" | "filter": (trainer, val/psnr at factor 1, PSNR at factor 4)}, the paths)"""
    paths = write_large_dataset(os.path.join(str(root), "data"))
    runs = {}
    for name, kwargs in (("plain", {}), ("filter", dict(filter3d=Filter3DConfig()))):
        trainer = make_trainer(paths, os.path.join(str(root), name), regularise=False, log_loss_interval=10 ** 6, log_metrics_interval=10 ** 6,
                               seed=0, **PROTOCOL, **kwargs)
        trainer.train()
        iteration, means = trainer.last_validation
        assert iteration == PROTOCOL["val_interval"]
        # (a render normalises the quaternions of the rows in camera in place, so a second one may differ in the last bits)
        assert abs(psnr_at(trainer, 1) - means["psnr"]) < 1e-3
        runs[name] = (trainer, means["psnr"], psnr_at(trainer, SCALE))
    return runs, paths


def psnr_under_the_training_filter(trainer):
    """the paper's own reading of its protocol: the full-size validation views under the filter the run was trained with, that
    of factor SCALE, instead of the narrower one of factor 1"""
    total = 0.0
    with torch.no_grad():
        features = trainer.filter3d.features(SCALE)
        for view in range(len(trainer.val_dataset)):
            image_gt, q, t, info = trainer.val_targets.target(view, 1)
            image = trainer.rasterisation(Rast.GaussianPointCloudRasterisationInput(
                point_cloud=trainer.scene.point_cloud, point_cloud_features=features, point_object_id=trainer.scene.point_object_id,
                point_invalid_mask=trainer.scene.point_invalid_mask, camera_info=info, q_pointcloud_camera=q, t_pointcloud_camera=t,
                color_max_sh_band=3))[0]
            total += trainer._metrics(torch.clamp(image, 0, 1).permute(2, 0, 1), image_gt)[1].item()
    return total / len(trainer.val_dataset)


def test_trained_at_a_quarter_validated_at_full_resolution(tmp_path):
    """Two runs of 120 iterations from the perturbed scene at a fixed factor 4 (64x96 frames of 256x384 pictures), the same
    seed and view order, validated at factor 1: without the filter and with Filter3DConfig().

    Measured on an MI355X (profiles/filter3d_margins.json, written by this test under GS_FILTER3D_MARGINS_OUT): val/psnr at
    factor 1 34.537 dB without the filter and 30.914 dB with it; at factor 4 37.419 and 33.792 dB.  So short a run on a scene of
    blobs does not separate the two in the filter's favour: the pictures were rendered from Gaussians of about half a training
    pixel WITHOUT a 3D filter, the initial scene has their scales already, and under the filter of factor 4 (about as wide as
    the Gaussians themselves: k / rate = 0.039 against a scale of 0.048) every one of them starts a quarter wider and at half
    its opacity, which 120 iterations do not undo.  Asserted instead, as the issue has it for this outcome: the factor-4 PSNR
    with the filter stays within the measured gap (3.627 dB, plus a tenth) of the run without it."""
    runs, paths = protocol(tmp_path)
    (tp, plain_1, plain_4), (tf, filter_1, filter_4) = runs["plain"], runs["filter"]
    assert tp.view_order == tf.view_order
    trained_1 = psnr_under_the_training_filter(tf)
    print(f"val/psnr at factor 1: {plain_1:.3f} without the filter, {filter_1:.3f} with it; at factor {SCALE}: {plain_4:.3f} and {filter_4:.3f}; "
          f"at factor 1 under the filter of factor {SCALE}: {trained_1:.3f}")
    out = os.environ.get("GS_FILTER3D_MARGINS_OUT")
    if out:
        with open(out, "w") as fh:
            json.dump(dict(schedule=PROTOCOL, pictures=[TU.H * SCALE, TU.W * SCALE], variance=0.2,
                           val_psnr_factor_1=dict(plain=plain_1, filter=filter_1), val_psnr_factor_4=dict(plain=plain_4, filter=filter_4),
                           val_psnr_factor_1_under_the_filter_of_factor_4=trained_1,
                           separates=bool(filter_1 > plain_1),
                           asserted=("val/psnr at factor 1 with the filter above the midpoint of the two recorded runs" if SEPARATES else
                                     f"the run does not separate the two at factor 1; asserted: PSNR at factor {SCALE} with the filter within "
                                     f"{GAP_DB:.3f} dB (the recorded gap plus a tenth) of the run without it")), fh, indent=1)
    assert all(np.isfinite(v) for v in (plain_1, plain_4, filter_1, filter_4, trained_1))
    if SEPARATES:
        assert filter_1 > (MEASURED["val_psnr_factor_1"]["plain"] + MEASURED["val_psnr_factor_1"]["filter"]) / 2
    else:
        assert plain_4 - filter_4 <= GAP_DB
    # the table files beside the scene files, and back
    model, k = tf.config.output_model_dir, PROTOCOL["val_interval"]
    for name in (f"scene_{k}.parquet", f"filter3d_{k}.pt", "best_scene.parquet", "best_filter3d.pt"):
        assert os.path.exists(os.path.join(model, name)), name
    assert not any("filter3d" in f for f in os.listdir(tp.config.output_model_dir))
    scene = GaussianPointCloudScene.from_parquet(os.path.join(model, f"scene_{k}.parquet"), device=DEV)
    loaded = Filter3D.load(os.path.join(model, f"filter3d_{k}.pt"), scene)
    valid = tf.scene.point_invalid_mask == 0
    assert torch.equal(loaded.rate.view(torch.int32), tf.filter3d.rate[valid].view(torch.int32)) and loaded.views is None
    assert (loaded.config.variance, loaded.config.margin, loaded.near, loaded.width, loaded.height) == (0.2, 0.15, 0.8, TU.W * SCALE, TU.H * SCALE)
    # the parquet stays raw: log-scales, logits and colours as the parameter holds them (the quaternions of the live scene have
    # been normalised again by the renders since the file was written, which may move them by an ulp)
    live = tf.scene.point_cloud_features.detach()[valid]
    assert torch.equal(scene.point_cloud_features[:, 4:], live[:, 4:])
    assert float((scene.point_cloud_features.detach()[:, :4] - live[:, :4]).abs().max()) < 1e-6
    with_views = Filter3D.load(os.path.join(model, "best_filter3d.pt"), scene, with_views=True)
    assert torch.equal(with_views.views, tf.filter3d.views)
    refreshed = with_views.refresh()                            # (the saved rates are those of iteration 100, the scene is that of 119)
    assert refreshed.shape == loaded.rate.shape and bool(torch.isfinite(refreshed).all()) and bool((refreshed > 0).all())


def test_the_renderer_applies_a_saved_table(data, tmp_path):
    from taichi_3d_gaussian_splatting_amd.GaussianPointRenderer import GaussianPointRenderer
    trainer = make_trainer(data["paths"], tmp_path, num_iterations=2, initial_downsample_factor=1, filter3d=Filter3DConfig(), seed=3)
    trainer.train()
    trainer.validation(2)
    model = trainer.config.output_model_dir
    cloud, table = os.path.join(model, "scene_2.parquet"), os.path.join(model, "filter3d_2.pt")
    poses = torch.stack([torch.tensor(r["T_pointcloud_camera"], dtype=torch.float32) for r in json.load(open(data["paths"]["val"]))])
    K = torch.tensor(TU.ground_truth_scene().camera_intrinsics)

    def renderer(**kw):
        config = GaussianPointRenderer.GaussianPointRendererConfig(cloud, poses, device=DEV, image_height=TU.H, image_width=TU.W, camera_intrinsics=K)
        return GaussianPointRenderer(config, **kw)
    plain, filtered, wide = renderer(), renderer(filter3d=table), renderer(filter3d=table, filter3d_factor=4)
    assert plain.filter3d is None and filtered.filter3d.views is None
    assert torch.equal(filtered.filter3d.rate.view(torch.int32), trainer.filter3d.rate.view(torch.int32))
    q_rows, t_rows = plain.pose_rows()
    images = [r.render(q_rows[0], t_rows[0])[0] for r in (plain, filtered, wide)]
    # what the table does to the frame: the features under the filter of factor 1, through the same rasteriser
    again = renderer()
    features = Filter3D.load(table, again.scene).features(1).detach()
    again.scene.point_cloud_features.data.copy_(features)
    assert torch.equal(images[1].view(torch.int32), again.render(q_rows[0], t_rows[0])[0].view(torch.int32))
    assert not torch.equal(images[0], images[1]) and not torch.equal(images[1], images[2])
    with pytest.raises(ValueError, match="single scene"):
        GaussianPointRenderer(GaussianPointRenderer.GaussianPointRendererConfig([cloud, cloud], poses, device=DEV, image_height=TU.H,
                                                                                image_width=TU.W, camera_intrinsics=K), filter3d=table)
