"""A tiny image dataset for the trainer tests and tools/trainer_smoke.py: a synthetic.synth scene rendered by the rasteriser
from a few poses, quantised to uint8 PNGs, with the reference's dataset JSONs and an initial cloud beside them."""
import json
import os

import numpy as np
import torch

H, W = 64, 96
N_POINTS = 400
TRAIN_VIEWS, VAL_VIEWS = (0, 1, 3, 4, 6, 7), (2, 5)


def ground_truth_scene():
    from taichi_3d_gaussian_splatting_amd.synthetic import synth
    return synth(N_POINTS, W, H, 0.08, sh_deg=3, seed=0)


def perturbed(scene, position_sigma=0.02, colour_sigma=0.3, seed=1):
    """-> (point_cloud, features) of the scene with noise on the positions and on the SH DC terms (columns 8, 24, 40)"""
    rng = np.random.default_rng(seed)
    pc = scene.point_cloud + rng.normal(0.0, position_sigma, scene.point_cloud.shape).astype(np.float32)
    ft = scene.point_cloud_features.copy()
    ft[:, [8, 24, 40]] += rng.normal(0.0, colour_sigma, (ft.shape[0], 3)).astype(np.float32)
    return pc, ft


def write_dataset(root, device="cuda:0", initial=None):
    """Renders the views into root/images, writes root/train.json, root/val.json and root/point_cloud.parquet (the ground-truth
    scene, or `initial` = (point_cloud, features)).  -> dict of the three paths and the uint8 images by view"""
    import PIL.Image
    from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast, scene_io
    from taichi_3d_gaussian_splatting_amd.synthetic import scene_input, view_pose
    from taichi_3d_gaussian_splatting_amd.utils import quaternion_to_rotation_matrix_torch
    root = str(root)
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    scene = ground_truth_scene()
    module = Rast(Rast.GaussianPointCloudRasterisationConfig())
    n_views = len(TRAIN_VIEWS) + len(VAL_VIEWS)
    records, images = {}, {}
    with torch.no_grad():
        for view in range(n_views):
            q, t = view_pose(view, n_views)
            image = module(scene_input(scene, q, t, device, band=3))[0]
            u8 = (image.clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy()
            path = os.path.join(root, "images", f"view_{view}.png")
            PIL.Image.fromarray(u8).save(path)
            T = np.eye(4)
            T[:3, :3] = quaternion_to_rotation_matrix_torch(torch.tensor(q, dtype=torch.float64))[0].numpy()
            T[:3, 3] = t[0]
            records[view] = dict(image_path=path, T_pointcloud_camera=T.tolist(), camera_intrinsics=scene.camera_intrinsics.tolist(),
                                 camera_height=H, camera_width=W, camera_id=0)
            images[view] = u8
    paths = dict(train=os.path.join(root, "train.json"), val=os.path.join(root, "val.json"), cloud=os.path.join(root, "point_cloud.parquet"))
    for name, views in (("train", TRAIN_VIEWS), ("val", VAL_VIEWS)):
        with open(paths[name], "w") as fh:
            json.dump([records[v] for v in views], fh)
    pc, ft = initial if initial is not None else (scene.point_cloud, scene.point_cloud_features)
    scene_io.save_parquet(paths["cloud"], pc, ft)
    return dict(paths=paths, images=images)


# Densification within an 8-iteration run of the 400-point scene (600 rows) at downsample factor 2 (32x48): a cycle at
# iterations 2, 4 and 6, floater removal from iteration 4 on.  Chosen with a CPU loop of density_loop_case.py's kind on this scene
# (the oracle's renders as targets, resized as the host target path does; loss_ref's L1+SSIM and regulariser; torch.optim.Adam at
# the learning rates of test_gpu_trainer.py; view order of seed 3).  There the three cycles fill 84, 142 and 113 rows (over- and
# under-reconstructed ones both, the last one cut short by a full scene), the first prunes 104 transparent rows, the second 35
# floaters, and the valid count goes 400 -> 380 -> 487 -> 600.
DENSIFY_SCENE = dict(max_num_points_ratio=1.5)
DENSIFY_CONTROLLER = dict(num_iterations_warm_up=2, num_iterations_densify=2, iteration_start_remove_floater=3,
                          densification_view_space_position_gradients_threshold=4e-4, under_reconstructed_num_pixels_threshold=25,
                          floater_near_camrea_num_pixels_threshold=25, floater_depth_threshold=6.0)


def train_config(paths, out_dir, densify=False, **overrides):
    """a TrainConfig on the dataset, nothing printed.  densify=False: densification off (the controller's warm-up lies beyond
    any run here); densify=True: DENSIFY_SCENE and DENSIFY_CONTROLLER"""
    from taichi_3d_gaussian_splatting_amd.GaussianPointTrainer import GaussianPointCloudTrainer
    config = GaussianPointCloudTrainer.TrainConfig(
        train_dataset_json_path=paths["train"], val_dataset_json_path=paths["val"], pointcloud_parquet_path=paths["cloud"],
        summary_writer_log_dir=os.path.join(str(out_dir), "logs"), output_model_dir=os.path.join(str(out_dir), "model"))
    config.adaptive_controller_config.num_iterations_warm_up = 10 ** 6
    if densify:
        for sub, values in ((config.gaussian_point_cloud_scene_config, DENSIFY_SCENE), (config.adaptive_controller_config, DENSIFY_CONTROLLER)):
            for name, value in values.items():
                assert hasattr(sub, name), name
                setattr(sub, name, value)
    for name, value in overrides.items():
        assert hasattr(config, name), name
        setattr(config, name, value)
    return config


SMOKE = dict(initial_downsample_factor=2, half_downsample_factor_interval=40, num_iterations=120, val_interval=119,
             feature_learning_rate=5e-3, position_learning_rate=1e-4)


def smoke_run(root, device="cuda:0"):
    """The 'it trains' run: from the perturbed ground truth, 120 iterations at factor 2 -> 1 (halving at 40), validation before
    and at the last iteration.  -> (trainer, means before, means after)"""
    from taichi_3d_gaussian_splatting_amd.GaussianPointTrainer import GaussianPointCloudTrainer, JsonlSummaryWriter
    data = write_dataset(os.path.join(str(root), "data"), device, initial=perturbed(ground_truth_scene()))
    config = train_config(data["paths"], os.path.join(str(root), "run"), **SMOKE)
    config.loss_function_config.enable_regularization = False       # the scale regulariser pulls a converged scene away from its images
    trainer = GaussianPointCloudTrainer(config, device=device, writer=JsonlSummaryWriter(config.summary_writer_log_dir))
    before = trainer.validation(0)
    trainer.train()
    iteration, after = trainer.last_validation
    assert iteration == SMOKE["val_interval"]
    return trainer, before, after
