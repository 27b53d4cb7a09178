"""GPU (-m gpu): GaussianPointCloudTrainer(density="mcmc") on tests/trainer_util.py's tiny dataset (400 points in 600 rows):
40 iterations with a refinement at 20 and at 30 (refine_start=10, refine_every=10: the iterations i with 10 < i, i % 10 == 0).
The valid count after each refinement is exactly min(cap, v + v * 50 / 1000), it never passes cap_max, the scene holds no NaN,
and the strategy's pieces are where the trainer says.  That "adaptive" is untouched is what tests/test_gpu_trainer.py shows."""
import pytest
import torch

import trainer_util as TU
from taichi_3d_gaussian_splatting_amd.GaussianPointTrainer import GaussianPointCloudTrainer, JsonlSummaryWriter
from taichi_3d_gaussian_splatting_amd.mcmc import COUNTS, MCMCConfig

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RUN = dict(num_iterations=40, val_interval=10 ** 6, initial_downsample_factor=2, half_downsample_factor_interval=10 ** 6,
           feature_learning_rate=5e-3, position_learning_rate=1e-4)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    return TU.write_dataset(tmp_path_factory.mktemp("trainer_mcmc_data"), DEV, initial=TU.perturbed(TU.ground_truth_scene()))


def make_trainer(data, out_dir, cap_max, **overrides):
    config = TU.train_config(data["paths"], out_dir, **dict(RUN, **overrides))
    config.gaussian_point_cloud_scene_config.max_num_points_ratio = 1.5
    return GaussianPointCloudTrainer(config, device=DEV, writer=JsonlSummaryWriter(config.summary_writer_log_dir), density="mcmc",
                                     mcmc_config=MCMCConfig(cap_max=cap_max, refine_start=10, refine_every=10, seed=3))


@pytest.mark.parametrize("cap_max", [None, 430])
def test_mcmc_run_grows_by_a_twentieth_per_refinement_up_to_the_cap(data, tmp_path, cap_max):
    trainer = make_trainer(data, tmp_path, cap_max)
    assert trainer.adaptive_controller is None and trainer.rasterisation._hook is None and trainer.density == "mcmc"
    n = trainer.scene.point_cloud.shape[0]
    assert n == 600 and int((trainer.scene.point_invalid_mask == 0).sum()) == TU.N_POINTS == 400
    before = trainer.scene.point_cloud.detach().clone()
    trainer.train()
    history = [(it, dict(zip(COUNTS, (int(x) for x in counts.cpu())))) for it, counts in trainer.mcmc.history]
    assert [it for it, _ in history] == [20, 30] and trainer.mcmc.refinement_calls == 2
    cap = n if cap_max is None else cap_max
    valid = TU.N_POINTS
    for it, c in history:
        print(it, c)
        assert c["valid_before"] == valid
        valid = min(cap, valid + valid * 50 // 1000)
        assert c["valid_after"] == valid <= cap and c["new"] == c["valid_after"] - c["valid_before"]
        assert c["destinations"] == c["dead"] + c["new"] and c["alive"] + c["dead"] == c["valid_before"] and 0 < c["sources"] <= c["destinations"]
    assert valid == (441 if cap_max is None else 430)
    mask = trainer.scene.point_invalid_mask
    assert int((mask == 0).sum()) == valid and int((mask == 1).sum()) == n - valid
    for t in (trainer.scene.point_cloud, trainer.scene.point_cloud_features):
        assert bool(torch.isfinite(t.detach()).all())
    assert not torch.equal(trainer.scene.point_cloud.detach()[:TU.N_POINTS], before[:TU.N_POINTS])
    # the regulariser ran on the last iteration's valid rows: its count, and two positive terms
    terms = trainer.mcmc.last_regulariser.cpu().tolist()
    assert terms[2] == valid and terms[0] > 0 and terms[1] > 0
    # the optimisers whose moments the strategy zeroes are the trainer's
    assert trainer.mcmc.optimizer is trainer.optimizer and trainer.mcmc.position_optimizer is trainer.position_optimizer


def test_mcmc_refuses_the_row_selective_step_and_unknown_settings(data, tmp_path):
    with pytest.raises(ValueError, match="sparse_adam"):
        make_trainer(data, tmp_path, None, sparse_adam=True)
    config = TU.train_config(data["paths"], tmp_path, **RUN)
    with pytest.raises(ValueError, match="density"):
        GaussianPointCloudTrainer(config, device=DEV, writer=JsonlSummaryWriter(config.summary_writer_log_dir), density="split")
    with pytest.raises(ValueError, match="mcmc_config"):
        GaussianPointCloudTrainer(config, device=DEV, writer=JsonlSummaryWriter(config.summary_writer_log_dir), mcmc_config=MCMCConfig())
