"""GPU (-m gpu): camera pose refinement in GaussianPointCloudTrainer (pose_table.py) on tiny synthetic image sets.

  (a) pose_refinement=None, and a config whose start_iteration lies beyond the run, are test_gpu_trainer.py's hand-written loop
      bit for bit;
  (b) the first refined iteration is the step written out by hand, and the scene's gradients are the unrefined run's;
  (c) on views with planted pose noise (tests/pose_trainer_util.py: an arc with a real baseline) refinement brings the training
      L1 below the midpoint of the clean and the noisy unrefined runs and the relative pose errors below the planted ones;
  (d) refine_pose aligns one view against the frozen ground-truth scene and leaves the controller alone;
  (e) the saved file, write_dataset and gaussian_point_render.py --pose_table agree;
  (f) it runs with filter3d, a sky and fixed-budget densification.

The schedule of (c) is trainer_util.SMOKE, 120 iterations: 20 Adam steps per view at the table's default rates.  The figures of a
run are in profiles/pose_refine_margins.json (tools/bench_poses.py --margins-out)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pose_trainer_util as PU
import trainer_util as TU
from test_gpu_trainer import hand_written_loop
from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast, pose_table
from taichi_3d_gaussian_splatting_amd.GaussianPointTrainer import GaussianPointCloudTrainer, JsonlSummaryWriter
from taichi_3d_gaussian_splatting_amd.LossFunction import LossFunction
from taichi_3d_gaussian_splatting_amd.pose_table import PoseRefinementConfig, PoseTable

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    return TU.write_dataset(tmp_path_factory.mktemp("pose_trainer_data"), DEV)


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """the three runs of (c), once"""
    return PU.planted_noise_runs(tmp_path_factory.mktemp("pose_planted"), DEV)


def make_trainer(data, out_dir, trainer_args=None, **overrides):
    config = TU.train_config(data["paths"], out_dir, **overrides)
    return GaussianPointCloudTrainer(config, device=DEV, writer=JsonlSummaryWriter(config.summary_writer_log_dir), **(trainer_args or {}))


@pytest.mark.parametrize("pose_refinement", [None, PoseRefinementConfig(start_iteration=6), PoseRefinementConfig(start_iteration=1000)],
                         ids=["none", "starts_at_the_end", "starts_beyond"])
def test_defaults_are_the_hand_written_loop(data, tmp_path, pose_refinement):
    n_it, band_interval, decay_interval, rate = 6, 2, 2, 0.9
    trainer = make_trainer(data, tmp_path, dict(pose_refinement=pose_refinement), num_iterations=n_it, initial_downsample_factor=1,
                           increase_color_max_sh_band_interval=band_interval, position_learning_rate_decay_interval=decay_interval,
                           position_learning_rate_decay_rate=rate, position_learning_rate=1e-4, seed=3)
    trainer.train()
    scene, _, op = hand_written_loop(data, trainer.config, trainer.view_order, n_it, band_interval, decay_interval, rate, False, seed=3)
    assert op.lr == trainer.position_optimizer.lr
    assert torch.equal(trainer.scene.point_cloud, scene.point_cloud)
    assert torch.equal(trainer.scene.point_cloud_features, scene.point_cloud_features)
    if pose_refinement is None:
        assert trainer.pose_table is None
    else:
        assert not bool(trainer.pose_table.delta.any()) and trainer.pose_table.steps == [0] * len(TU.TRAIN_VIEWS)


def test_first_refined_iteration_is_the_step_by_hand(data, tmp_path):
    kwargs = dict(num_iterations=1, initial_downsample_factor=1, position_learning_rate=1e-4, seed=3)
    config = PoseRefinementConfig(lr=2e-3, reg=0.25)
    refined = make_trainer(data, tmp_path / "refined", dict(pose_refinement=config), **kwargs)
    plain = make_trainer(data, tmp_path / "plain", **kwargs)
    start = [t.detach().clone() for t in (plain.scene.point_cloud, plain.scene.point_cloud_features)]
    refined.train()
    plain.train()
    view = refined.view_order[0]
    assert plain.view_order[0] == view
    # a correction of zeros is the dataset's pose bit for bit: the scene saw the same frame, and got the same gradients and step
    for a, b in ((refined.scene.point_cloud, plain.scene.point_cloud), (refined.scene.point_cloud_features, plain.scene.point_cloud_features)):
        assert torch.equal(a.grad, b.grad) and bool(a.grad.any()) and torch.equal(a, b)
    # the pose's step by hand, on the scene as it was
    image_gt, q, t, camera_info = plain.train_targets.target(view, 1)
    module = Rast(Rast.GaussianPointCloudRasterisationConfig())
    ql, tl = q.clone().requires_grad_(True), t.clone().requires_grad_(True)
    inp = Rast.GaussianPointCloudRasterisationInput(
        point_cloud=start[0], point_cloud_features=start[1], point_object_id=plain.scene.point_object_id,
        point_invalid_mask=plain.scene.point_invalid_mask, camera_info=camera_info, q_pointcloud_camera=ql, t_pointcloud_camera=tl,
        color_max_sh_band=0)
    LossFunction(LossFunction.LossFunctionConfig())(module(inp)[0].permute(2, 0, 1), image_gt, clamp_predicted=True)[0].backward()
    by_hand = PoseTable(len(TU.TRAIN_VIEWS), DEV, config)
    by_hand.grad[view] = pose_table.compose_backward(q[None], by_hand.delta[view:view + 1], ql.grad[None].contiguous(), tl.grad[None].contiguous(),
                                                     config.reg)[0]
    assert torch.equal(refined.pose_table.grad[view], by_hand.grad[view]) and bool(by_hand.grad[view].any())
    by_hand.step(view, 0)
    assert torch.equal(refined.pose_table.delta, by_hand.delta) and refined.pose_table.steps == by_hand.steps
    assert torch.equal(refined.pose_table.exp_avg, by_hand.exp_avg) and torch.equal(refined.pose_table.exp_avg_sq, by_hand.exp_avg_sq)
    # Adam's first step is lr * sign(g) (|g| >> eps): every float of the view's row moved by the learning rate, against its gradient
    g = by_hand.grad[view].double()
    want = -config.lr_at(0) * g / (g.abs() + config.eps)
    assert torch.allclose(by_hand.delta[view].double(), want, rtol=1e-5, atol=0)
    others = [v for v in range(len(TU.TRAIN_VIEWS)) if v != view]
    assert not bool(refined.pose_table.delta[others].any())


def test_planted_noise_is_refined_away(planted):
    m = planted["margins"]
    print(json.dumps(m, indent=1))
    assert m["l1_clean"] < m["l1_noisy"]                                                # the planted noise costs something
    assert m["l1_refined"] < 0.5 * (m["l1_clean"] + m["l1_noisy"])                      # below the midpoint of the two unrefined runs
    assert m["rotation_error_refined"] < m["rotation_error_planted"]                    # radians, mean over all pairs of views
    assert m["translation_error_refined"] < m["translation_error_planted"]
    assert np.isfinite(m["val_psnr"]) and np.isfinite(m["val_psnr_aligned"])


def test_refine_pose_aligns_one_view_and_leaves_the_controller_alone():
    from taichi_3d_gaussian_splatting_amd import GaussianPointAdaptiveController
    from taichi_3d_gaussian_splatting_amd.synthetic import scene_input
    scene = TU.ground_truth_scene()
    truth = PU.true_pose(3)
    q_true, t_true = PU.matrix_to_qt(truth)
    inp = scene_input(scene, q_true, t_true, DEV, band=3)
    controller = GaussianPointAdaptiveController(
        config=GaussianPointAdaptiveController.GaussianPointAdaptiveControllerConfig(),
        maintained_parameters=GaussianPointAdaptiveController.GaussianPointAdaptiveControllerMaintainedParameters(
            pointcloud=inp.point_cloud, pointcloud_features=inp.point_cloud_features, point_invalid_mask=inp.point_invalid_mask,
            point_object_id=inp.point_object_id))
    module = Rast(Rast.GaussianPointCloudRasterisationConfig(), backward_valid_point_hook=controller.update)
    module.track_touched_rows = True
    with torch.no_grad():
        target = module(inp)[0].permute(2, 0, 1).contiguous()
    offset = np.eye(4)
    offset[:3, :3], offset[:3, 3] = PU.rotation_exp([0.004, -0.006, 0.003]), [0.04, -0.02, 0.03]
    q0, t0 = PU.matrix_to_qt(truth @ offset)
    import dataclasses
    start = dataclasses.replace(inp, q_pointcloud_camera=torch.tensor(q0, device=DEV), t_pointcloud_camera=torch.tensor(t0, device=DEV))
    sentinel = object()
    module.last_touched_rows = sentinel
    counter = controller.iteration_counter
    accumulators = {k: v.clone() for k, v in vars(controller.accumulators).items() if isinstance(v, torch.Tensor)}
    assert len(accumulators) == 6

    def l1(q, t):
        with torch.no_grad():
            image = module(dataclasses.replace(inp, q_pointcloud_camera=q, t_pointcloud_camera=t))[0].permute(2, 0, 1)
            return float((image.clamp(0, 1) - target.clamp(0, 1)).abs().mean())

    def pose_error(q, t):
        T = np.eye(4)
        from taichi_3d_gaussian_splatting_amd.utils import quaternion_to_rotation_matrix_torch
        qd = q.detach().cpu().double()
        T[:3, :3] = quaternion_to_rotation_matrix_torch(qd / qd.norm())[0].numpy()
        T[:3, 3] = t.detach().cpu().double().numpy()[0]
        return PU.relative_pose_errors([np.eye(4), T], [np.eye(4), truth])

    before_l1, before_err = l1(start.q_pointcloud_camera, start.t_pointcloud_camera), pose_error(start.q_pointcloud_camera, start.t_pointcloud_camera)
    q, t, delta = pose_table.refine_pose(module, start, target, steps=60, lr=2e-3)
    after_l1, after_err = l1(q, t), pose_error(q, t)
    print(f"refine_pose: L1 {before_l1:.5f} -> {after_l1:.5f}, rotation {before_err[0]:.5f} -> {after_err[0]:.5f} rad, "
          f"translation {before_err[1]:.5f} -> {after_err[1]:.5f}")
    assert q.shape == (1, 4) and t.shape == (1, 3) and delta.shape == (6,) and not q.requires_grad and bool(delta.any())
    assert after_l1 < before_l1 and after_err[0] < before_err[0] and after_err[1] < before_err[1]
    # the corrected pose is the six floats composed onto the start
    qc, tc = pose_table.compose_forward(start.q_pointcloud_camera[None], start.t_pointcloud_camera[None], delta[None])
    assert torch.equal(qc[0], q) and torch.equal(tc[0], t)
    # pose-only backwards: no hook call, no statistics, and the touched rows are what they were
    assert controller.iteration_counter == counter and module.last_touched_rows is sentinel
    for name, value in accumulators.items():
        assert torch.equal(getattr(controller.accumulators, name), value), name
    assert inp.point_cloud.grad is None and inp.point_cloud_features.grad is None


def test_files_write_dataset_and_the_renderer_agree(planted, tmp_path):
    run = planted["refined"]
    model_dir, paths = run["model_dir"], planted["noisy_paths"]
    last = os.path.join(model_dir, f"poses_{PU.PLANTED_SCHEDULE['val_interval']}.pt")
    assert os.path.exists(last) and os.path.exists(os.path.join(model_dir, "best_poses.pt"))
    table, image_paths = PoseTable.load(last, DEV)
    assert image_paths == run["image_paths"] and torch.equal(table.delta, run["delta"].to(DEV)) and bool(table.delta.any(dim=1).all())
    # a file of three of the six views
    some = [0, 2, 5]
    part = str(tmp_path / "some_poses.pt")
    torch.save(dict(delta=table.delta[some].cpu(), exp_avg=table.exp_avg[some].cpu(), exp_avg_sq=table.exp_avg_sq[some].cpu(),
                    steps=[table.steps[v] for v in some], image_paths=[image_paths[v] for v in some]), part)
    dst = str(tmp_path / "refined_train.json")
    assert pose_table.write_dataset(part, paths["train"], dst) == 3
    src_records, dst_records = json.load(open(paths["train"])), json.load(open(dst))
    # on the device, from the float32 poses the trainer reads
    from taichi_3d_gaussian_splatting_amd.ImagePoseDataset import ImagePoseDataset
    from taichi_3d_gaussian_splatting_amd.utils import quaternion_to_rotation_matrix_torch
    dataset = ImagePoseDataset(dataset_json_path=paths["train"])
    for v in range(len(src_records)):
        same = np.array_equal(np.asarray(src_records[v]["T_pointcloud_camera"]), np.asarray(dst_records[v]["T_pointcloud_camera"]))
        assert same == (v not in some)
        if v in some:
            _, q, t, _ = dataset.load_raw(v)
            qc, tc = pose_table.compose_forward(q.to(DEV).reshape(1, 1, 4), t.to(DEV).reshape(1, 1, 3), table.delta[v:v + 1])
            T = np.asarray(dst_records[v]["T_pointcloud_camera"])
            R = quaternion_to_rotation_matrix_torch(qc[0].double().cpu() / qc[0].double().cpu().norm())[0].numpy()
            assert np.abs(R - T[:3, :3]).max() < 5e-6 and np.abs(tc[0, 0].cpu().numpy() - T[:3, 3]).max() < 5e-6     # float32 poses
    # the renderer: corrected frames differ from the uncorrected ones exactly for the views in the file, and are the frames of
    # the dataset write_dataset wrote (to the 8 bits of a frame, but for pixels on a rounding edge)
    frames = {}
    scene = os.path.join(model_dir, f"scene_{PU.PLANTED_SCHEDULE['val_interval']}.parquet")
    for name, extra in (("plain", ["--poses", paths["train"]]), ("table", ["--poses", paths["train"], "--pose_table", part]),
                        ("written", ["--poses", dst])):
        out = tmp_path / name
        subprocess.check_call([sys.executable, os.path.join(ROOT, "gaussian_point_render.py"), "--parquet_path", scene, "--output_prefix", str(out),
                               "--format", "npy", "--device", DEV] + extra, cwd=ROOT, stdout=subprocess.DEVNULL)
        files = sorted(p for p in os.listdir(out) if p.endswith(".npy"))
        assert len(files) == len(src_records)
        frames[name] = [np.load(os.path.join(out, f)) for f in files]
    for v in range(len(src_records)):
        assert np.array_equal(frames["plain"][v], frames["table"][v]) == (v not in some), v
        close = np.abs(frames["table"][v].astype(np.int32) - frames["written"][v].astype(np.int32))
        assert close.max() <= 2 and (close > 0).mean() < 0.05, v


@pytest.mark.parametrize("combination", ["filter3d", "sky", "mcmc"])
def test_combinations_complete(data, tmp_path, combination):
    from taichi_3d_gaussian_splatting_amd.filter3d import Filter3DConfig
    from taichi_3d_gaussian_splatting_amd.mcmc import MCMCConfig
    from taichi_3d_gaussian_splatting_amd.utils import quaternion_to_rotation_matrix_torch
    args = dict(filter3d=dict(filter3d=Filter3DConfig(interval=4)), sky=dict(background="sky"),
                mcmc=dict(density="mcmc", mcmc_config=MCMCConfig(cap_max=430, seed=3)))[combination]
    config = TU.train_config(data["paths"], tmp_path, num_iterations=10, val_interval=9, initial_downsample_factor=2, position_learning_rate=1e-4,
                             seed=3)
    if combination == "mcmc":
        config.gaussian_point_cloud_scene_config.max_num_points_ratio = 1.5
    trainer = GaussianPointCloudTrainer(config, device=DEV, writer=JsonlSummaryWriter(config.summary_writer_log_dir),
                                        pose_refinement=PoseRefinementConfig(lr=2e-3, start_iteration=2), **args)
    table = trainer.pose_table
    checks = []
    if combination == "filter3d":
        # at every refresh of the rates the filter's view table is the one of table.corrected(), the intrinsics as they were
        first = trainer.filter3d.views.clone()
        refresh = trainer.filter3d.refresh

        def checking_refresh():
            rows = trainer.filter3d.views.cpu().numpy()
            q, t = table.corrected(trainer.train_targets.q, trainer.train_targets.t)
            ok = np.array_equal(rows[:, 12:], first.cpu().numpy()[:, 12:])
            for v in range(len(TU.TRAIN_VIEWS)):
                qd = q[v].double().cpu()
                R_pc = quaternion_to_rotation_matrix_torch((qd / qd.norm())[None])[0].numpy()
                ok = ok and np.abs(rows[v, :9].reshape(3, 3) - R_pc.T).max() < 1e-6
                ok = ok and np.abs(rows[v, 9:12] + R_pc.T @ t[v].double().cpu().numpy()).max() < 1e-5
            checks.append((bool(ok), not np.array_equal(rows, first.cpu().numpy())))
            return refresh()
        trainer.filter3d.refresh = checking_refresh
    trainer.train()
    assert sum(table.steps) == 8 and bool(table.delta.any()) and bool(torch.isfinite(table.delta).all())
    assert bool(torch.isfinite(trainer.scene.point_cloud).all()) and trainer.last_validation[0] == 9
    assert os.path.exists(os.path.join(trainer.config.output_model_dir, "poses_9.pt"))
    if combination == "filter3d":
        assert len(checks) >= 3 and all(ok for ok, _ in checks)          # iterations 0, 4 and 8
        assert not checks[0][1] and checks[-1][1]                        # the dataset's table at first, another once poses have moved
