"""A tiny image dataset for the pose-refinement tests and tools/bench_poses.py: trainer_util's synth scene seen from views on an
arc around it -- a real baseline, every camera looking at the scene's centre -- with seeded noise planted on the training poses.
(trainer_util's own views share one camera centre, which leaves translation against rotation ill-conditioned.)"""
import json
import os

import numpy as np
import torch

import trainer_util as TU

H, W = TU.H, TU.W
N_VIEWS = 8
TRAIN_VIEWS, VAL_VIEWS = (0, 1, 3, 4, 6, 7), (2, 5)
CENTRE = np.array([0.0, 0.0, 6.0])             # of synth()'s frustum of depths 2 .. 10
DEPTH = 6.0                                     # the scene depth: camera to centre
ARC_STEP_DEG = 4.0                              # between neighbouring views: a baseline of 0.42 per step
# planted noise per axis: |rotation| of the order of half a degree, |translation| of the order of 1 % of the scene depth
ROTATION_SIGMA = np.deg2rad(0.5) / np.sqrt(3.0)
TRANSLATION_SIGMA = 0.01 * DEPTH / np.sqrt(3.0)


def rotation_exp(w):
    """Rodrigues' formula, float64"""
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w)
    Wx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + Wx
    return np.eye(3) + np.sin(th) / th * Wx + (1.0 - np.cos(th)) / th ** 2 * (Wx @ Wx)


def true_pose(view):
    """-> the 4x4 float64 T_pointcloud_camera of a view: on a circle of radius DEPTH about CENTRE in the x-z plane, looking at it"""
    phi = np.deg2rad((view - (N_VIEWS - 1) / 2.0) * ARC_STEP_DEG)
    T = np.eye(4)
    T[:3, :3] = rotation_exp([0.0, phi, 0.0])
    T[:3, 3] = CENTRE - DEPTH * T[:3, 2]
    return T


def planted_noise(seed=7):
    """-> {training view: 4x4 D}: the rigid motion planted on the right of its true pose"""
    rng = np.random.default_rng(seed)
    out = {}
    for view in TRAIN_VIEWS:
        D = np.eye(4)
        D[:3, :3] = rotation_exp(rng.normal(0.0, ROTATION_SIGMA, 3))
        D[:3, 3] = rng.normal(0.0, TRANSLATION_SIGMA, 3)
        out[view] = D
    return out


def matrix_to_qt(T):
    """-> (q (1,4) xyzw, t (1,3)) float32 of a 4x4 pose, as ImagePoseDataset hands them out"""
    from taichi_3d_gaussian_splatting_amd.utils import SE3_to_quaternion_and_translation_torch
    q, t = SE3_to_quaternion_and_translation_torch(torch.tensor(np.asarray(T)[None], dtype=torch.float64))
    return q.to(torch.float32).numpy().reshape(1, 4), t.to(torch.float32).numpy().reshape(1, 3)


def relative_pose_errors(poses, truth):
    """Mean relative pose error over all pairs of views, float64: for i < j, E = (T_i^-1 T_j)^-1 (S_i^-1 S_j) with T the poses and
    S the truth; -> (mean rotation angle of E in radians, mean length of E's translation).  Free of the rigid motion a scene
    trained with its poses can absorb."""
    poses, truth = [np.asarray(p, dtype=np.float64) for p in poses], [np.asarray(p, dtype=np.float64) for p in truth]
    angles, lengths = [], []
    for i in range(len(poses)):
        for j in range(i + 1, len(poses)):
            E = np.linalg.inv(np.linalg.inv(poses[i]) @ poses[j]) @ (np.linalg.inv(truth[i]) @ truth[j])
            angles.append(np.arccos(np.clip((np.trace(E[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))
            lengths.append(np.linalg.norm(E[:3, 3]))
    return float(np.mean(angles)), float(np.mean(lengths))


def write_dataset(root, device="cuda:0", initial=None, noise=None):
    """Renders the arc views of the ground-truth scene under their TRUE poses into root/images; writes root/train.json (its poses
    with `noise`, {view: D}, planted on the right), root/val.json (true poses) and root/point_cloud.parquet (the ground truth, or
    `initial` = (point_cloud, features)).  -> dict(paths, truth: {view: 4x4}, written: {view: the 4x4 in the JSON})"""
    import PIL.Image
    from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast, scene_io
    from taichi_3d_gaussian_splatting_amd.synthetic import scene_input
    root = str(root)
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    scene = TU.ground_truth_scene()
    module = Rast(Rast.GaussianPointCloudRasterisationConfig())
    records, truth, written = {}, {}, {}
    with torch.no_grad():
        for view in range(N_VIEWS):
            truth[view] = true_pose(view)
            q, t = matrix_to_qt(truth[view])
            image = module(scene_input(scene, q, t, device, band=3))[0]
            u8 = (image.clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy()
            path = os.path.join(root, "images", f"view_{view}.png")
            PIL.Image.fromarray(u8).save(path)
            written[view] = truth[view] @ noise[view] if noise and view in noise else truth[view]
            records[view] = dict(image_path=path, T_pointcloud_camera=written[view].tolist(), camera_intrinsics=scene.camera_intrinsics.tolist(),
                                 camera_height=H, camera_width=W, camera_id=0)
    paths = dict(train=os.path.join(root, "train.json"), val=os.path.join(root, "val.json"), cloud=os.path.join(root, "point_cloud.parquet"))
    for name, views in (("train", TRAIN_VIEWS), ("val", VAL_VIEWS)):
        with open(paths[name], "w") as fh:
            json.dump([records[v] for v in views], fh)
    pc, ft = initial if initial is not None else (scene.point_cloud, scene.point_cloud_features)
    scene_io.save_parquet(paths["cloud"], pc, ft)
    return dict(paths=paths, truth=truth, written=written)


# trainer_util.SMOKE as it is: 120 iterations, factor 2 -> 1 at 40, validation at the last iteration; the table's default rates
PLANTED_SCHEDULE = dict(TU.SMOKE)
PLANTED_POSES = dict(lr=1e-3, lr_final=1e-4)
VALIDATION_POSE_STEPS = 30


def planted_noise_runs(root, device="cuda:0", schedule=None, poses=None, seed=7):
    """Three runs of the schedule from the perturbed ground truth: clean poses without refinement, noisy poses without, noisy
    poses with.  -> dict(margins: the figures of profiles/pose_refine_margins.json, refined: what the refined run left behind,
    noisy_paths: the noisy dataset's files)"""
    from taichi_3d_gaussian_splatting_amd.GaussianPointTrainer import GaussianPointCloudTrainer, JsonlSummaryWriter
    from taichi_3d_gaussian_splatting_amd.pose_table import PoseRefinementConfig
    schedule = dict(PLANTED_SCHEDULE if schedule is None else schedule)
    poses = dict(PLANTED_POSES if poses is None else poses)
    noise = planted_noise(seed)
    initial = TU.perturbed(TU.ground_truth_scene())
    data = {"clean": write_dataset(os.path.join(str(root), "clean"), device, initial=initial),
            "noisy": write_dataset(os.path.join(str(root), "noisy"), device, initial=initial, noise=noise)}
    runs = {}
    for name, images, refine in (("clean", "clean", False), ("noisy", "noisy", False), ("refined", "noisy", True)):
        config = TU.train_config(data[images]["paths"], os.path.join(str(root), "run_" + name), log_loss_interval=1, log_metrics_interval=10 ** 6,
                                 **schedule)
        config.loss_function_config.enable_regularization = False
        trainer = GaussianPointCloudTrainer(config, device=device, writer=JsonlSummaryWriter(config.summary_writer_log_dir),
                                            pose_refinement=PoseRefinementConfig(**poses) if refine else None,
                                            validation_pose_steps=VALIDATION_POSE_STEPS if refine else 0)
        trainer.train()
        iteration, means = trainer.last_validation
        assert iteration == schedule["val_interval"]
        trainer.writer.flush()
        l1 = [(r["step"], r["value"]) for r in JsonlSummaryWriter.read(trainer.writer.path) if r["tag"] == "train/l1 loss"]
        assert [s for s, _ in l1] == list(range(schedule["num_iterations"]))
        runs[name] = (trainer, means, float(np.mean([v for _, v in l1[-len(TRAIN_VIEWS):]])))
    trainer, means, _ = runs["refined"]
    assert runs["clean"][0].view_order == runs["noisy"][0].view_order == trainer.view_order
    assert sorted(trainer.view_order[schedule["num_iterations"] - len(TRAIN_VIEWS):schedule["num_iterations"]]) == list(range(len(TRAIN_VIEWS)))
    model_dir = trainer.config.output_model_dir
    table_file = os.path.join(model_dir, f"poses_{schedule['val_interval']}.pt")
    truth = [data["noisy"]["truth"][v] for v in TRAIN_VIEWS]
    planted_err = relative_pose_errors([data["noisy"]["written"][v] for v in TRAIN_VIEWS], truth)
    refined_err = relative_pose_errors(corrected_poses(table_file, data["noisy"]["paths"]["train"]), truth)
    margins = dict(schedule=schedule, poses=poses, validation_pose_steps=VALIDATION_POSE_STEPS, noise_seed=seed,
                   l1_clean=runs["clean"][2], l1_noisy=runs["noisy"][2], l1_refined=runs["refined"][2],
                   rotation_error_planted=planted_err[0], rotation_error_refined=refined_err[0],
                   translation_error_planted=planted_err[1], translation_error_refined=refined_err[1],
                   val_psnr_clean=runs["clean"][1]["psnr"], val_psnr_noisy=runs["noisy"][1]["psnr"], val_psnr=means["psnr"],
                   val_psnr_aligned=means["psnr_aligned"], val_ssim=means["ssim"], val_ssim_aligned=means["ssim_aligned"])
    refined = dict(model_dir=model_dir, image_paths=trainer.train_image_paths(), delta=trainer.pose_table.delta.detach().cpu().clone(),
                   steps=list(trainer.pose_table.steps))
    return dict(margins=margins, refined=refined, noisy_paths=data["noisy"]["paths"])


def corrected_poses(table_file, train_json):
    """-> the 4x4 float64 corrected pose of every training view, in the dataset's order (pose_table.corrected_matrices; a view
    that is not in the file keeps its pose)"""
    from taichi_3d_gaussian_splatting_amd import pose_table
    with open(train_json) as fh:
        records = json.load(fh)
    return [np.asarray(r["T_pointcloud_camera"], dtype=np.float64) if T is None else T
            for r, T in zip(records, pose_table.corrected_matrices(table_file, records))]
