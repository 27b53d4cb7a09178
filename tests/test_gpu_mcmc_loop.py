"""GPU (-m gpu): fixed-budget densification inside the training iteration -- MCMCStrategy.before_step between the backward and the
optimiser steps, after_step behind them -- against tests/mcmc_ref.py, one call at a time.

The run is tests/test_gpu_trainer_mcmc.py's trainer (400 points in 600 rows, factor 2, density="mcmc") for 12 iterations with
MCMCConfig(refine_start=2, refine_every=3, seed=3): refinements at iterations 3, 6 and 9, with call indices 0, 1 and 2.  The
position rate decays by 0.9 after every iteration, so the rate an iteration stepped with and the rate after its decay are
different numbers.  40 rows of the initial scene (tests/mcmc_cases.py, loop_initial) have logits spread over [-6, -2.5], on both
sides of logit(0.005): their noise gate is open, and some of them are dead at the first refinement.

The comparison is teacher-forced, as tests/test_gpu_density_loop.py's is.  MCMCStrategy.before_step and after_step are wrapped;
each wrapper copies what the call may change, makes the call, and compares the result with mcmc_ref fed the copies, so no
comparison carries the rounding of an earlier call.

before_step(i), with `added` the reference's regulariser term of the scene as it is: in columns 4..7 of the valid rows
|grad_after - (grad_before + added)| <= 4 ulp32(added) + 1/2 ulp32(grad_after) -- the 4 ulp of test_regulariser_against_float64 on the
term and the one f32 addition; every other element of the features' gradient, the positions' gradient, the scene and the four
moment tensors keep every bit; last_regulariser is within 1e-6 of the reference's two terms, with the exact valid count.

after_step(i, lr): lr is the rate FusedAdam.step() of the positions has just used (recorded by a wrapper around it), which is
position_learning_rate x 0.9^i.  The noise is mcmc_ref.noise(..., noise_lr x lr, seed 3, step_index=i): on the rows whose
products are all normal numbers |x_after - (x_before + delta)| <= 2e-5 magnitude + 1/2 ulp32(x_after) (test_noise_against_float64's
bar and the one addition); rows that do not move, the features, the mask, the object ids and the moments keep every bit.  At least
ten rows move by more than an ulp of their position in every iteration -- a condition of the test, asserted.  On a refinement
iteration the noise and the relocation happen in one call, so the wrapper runs mcmc.inject_noise itself on a clone of the
scene before the call (the same call from the same state gives the same bits: test_noise_against_float64), compares that with the
reference's noise, and takes it as the relocation's input: test_gpu_mcmc.py's check_relocate against mcmc_ref.relocate(seed=3,
call_index=the number of earlier refinements), the moments being exp_avg and exp_avg_sq of the trainer's two FusedAdams -- zero on
the touched rows, every bit kept elsewhere, state["step"] as it was.  history gains (i, counts), refinement_calls goes 0, 1, 2, 3.
On the other iterations the scene after the call is the clone's, bit for bit.

From the reference alone: the three refinements draw different source lists, and each differs from what another call index
(another refinement's, or the iteration) would have drawn from the same weights.

The device's counts on an MI355X (valid before / dead / alive / free / new / D / sources -> valid after):
  iteration 3 (call 0): 400 /  9 / 391 / 200 / 20 / 29 / 28 -> 420
  iteration 6 (call 1): 420 /  0 / 420 / 180 / 21 / 21 / 20 -> 441
  iteration 9 (call 2): 441 /  0 / 441 / 159 / 22 / 22 / 22 -> 463
The nine dead rows of iteration 3 are planted ones; the relocation lifts them to opacity 0.005 and none has died again by
iteration 6.  Rows moved by more than an ulp: 55, 55, 52, 53, 43, 46, 47, 44, 43, 46, 43, 46 over the twelve iterations.  The
relocated logits and log-scales are within 0.50 f32 ulp of the reference, the regulariser's addition uses 0.995 of its bound (the
half ulp of the addition is most of it).  The reference costs milliseconds at 600 rows; the whole test takes 4 s.

A strategy whose after_step is called behind the decay of the position rate (noise_lr x lr x 0.9), one that numbers the
relocations by the iteration (call_index=iteration), and one that takes the noise's counter from refinement_calls all pass
tests/test_gpu_trainer_mcmc.py, which asserts counts and finiteness; each fails here at the first iteration it differs."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mcmc_cases as MC
import mcmc_ref
import trainer_util as TU
from test_gpu_mcmc import bits, check_relocate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ITERATIONS, REFINEMENTS = 12, [3, 6, 9]
DECAY = 0.9
RUN = dict(num_iterations=ITERATIONS, val_interval=10 ** 6, initial_downsample_factor=2, half_downsample_factor_interval=10 ** 6,
           feature_learning_rate=5e-3, position_learning_rate=MC.LOOP["position_learning_rate"],
           position_learning_rate_decay_interval=1, position_learning_rate_decay_rate=DECAY)
SMALLEST_NORMAL = 2.0 ** -126


def ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def host(t):
    return None if t is None else t.detach().cpu().numpy().copy()


def scene_of(strategy):
    sc = strategy.scene
    return dict(pc=host(sc.point_cloud), ft=host(sc.point_cloud_features), mask=host(sc.point_invalid_mask), obj=host(sc.point_object_id))


def moments_of(strategy):
    """[features' exp_avg, exp_avg_sq, positions' exp_avg, exp_avg_sq] and the two step counts"""
    states = [strategy.optimizer.state[0], strategy.position_optimizer.state[0]]
    return [host(st[name]) for st in states for name in ("exp_avg", "exp_avg_sq")], [st["step"] for st in states]


def assert_same_bits(after, before, what):
    for name in before:
        assert np.array_equal(bits(after[name]), bits(before[name])), (what, name)


def assert_moments_kept(strategy, before, steps, what):
    after, steps_after = moments_of(strategy)
    assert steps_after == steps, what
    for a, b in zip(after, before):
        assert np.array_equal(bits(a), bits(b)), what


def position_rate_at(iteration):
    lr = MC.LOOP["position_learning_rate"]
    for _ in range(iteration):
        lr *= DECAY
    return lr


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    pc, ft, rows = MC.loop_initial(*TU.perturbed(TU.ground_truth_scene()))
    return TU.write_dataset(tmp_path_factory.mktemp("mcmc_loop_data"), DEV, initial=(pc, ft))


def test_strategy_in_the_loop_matches_the_reference_call_by_call(data, tmp_path, monkeypatch):
    from taichi_3d_gaussian_splatting_amd import mcmc
    from taichi_3d_gaussian_splatting_amd.GaussianPointTrainer import GaussianPointCloudTrainer, JsonlSummaryWriter
    from taichi_3d_gaussian_splatting_amd.mcmc import MCMCConfig, MCMCStrategy
    from taichi_3d_gaussian_splatting_amd.optim import FusedAdam
    config = TU.train_config(data["paths"], tmp_path, **RUN)
    config.gaussian_point_cloud_scene_config.max_num_points_ratio = 1.5
    mcmc_config = MCMCConfig(cap_max=None, refine_start=2, refine_every=3, seed=MC.LOOP["seed"])
    assert mcmc_config.noise_lr == MC.LOOP["noise_lr"] and [i for i in range(ITERATIONS) if mcmc_config.is_refinement(i)] == REFINEMENTS
    trainer = GaussianPointCloudTrainer(config, device=DEV, writer=JsonlSummaryWriter(config.summary_writer_log_dir), density="mcmc",
                                        mcmc_config=mcmc_config)
    log = dict(before=[], after=[], refinements=[])
    original = dict(before=MCMCStrategy.before_step, after=MCMCStrategy.after_step, step=FusedAdam.step)

    def step(self, *args, **kwargs):
        self.stepped_with = self.lr                                 # the rate this step uses
        return original["step"](self, *args, **kwargs)

    def before_step(self, iteration):
        assert self is trainer.mcmc and iteration == len(log["before"]) == len(log["after"])
        s = scene_of(self)
        grads = dict(ft=host(self.scene.point_cloud_features.grad), pc=host(self.scene.point_cloud.grad))
        mom, steps = moments_of(self)
        original["before"](self, iteration)
        value, added = mcmc_ref.regulariser(s["ft"], s["mask"], mcmc_config.opacity_reg, mcmc_config.scale_reg)
        after = host(self.scene.point_cloud_features.grad)
        checked = np.zeros(after.shape, bool)
        checked[s["mask"] == 0, 4:8] = True
        assert (added[checked] > 0).all() and not added[~checked].any()
        want = grads["ft"].astype(np.float64) + added
        err = np.abs(after.astype(np.float64) - want)
        bound = 4.0 * ulp32(added) + 0.5 * ulp32(after)
        assert (err[checked] <= bound[checked]).all(), float((err[checked] / bound[checked]).max())
        assert (bits(after)[checked] != bits(grads["ft"])[checked]).any()
        assert np.array_equal(bits(after)[~checked], bits(grads["ft"])[~checked])
        assert np.array_equal(bits(host(self.scene.point_cloud.grad)), bits(grads["pc"]))
        assert_same_bits(scene_of(self), s, "before_step")
        assert_moments_kept(self, mom, steps, "before_step")
        out = self.last_regulariser.cpu().numpy().astype(np.float64)
        assert out[2] == value[2] == (s["mask"] == 0).sum() and (np.abs(out[:2] - value[:2]) <= 1e-6 * np.abs(value[:2])).all()
        log["before"].append(float((err[checked] / bound[checked]).max()))

    def after_step(self, iteration, position_lr):
        assert self is trainer.mcmc and iteration == len(log["after"]) == len(log["before"]) - 1
        assert position_lr == self.position_optimizer.stepped_with == position_rate_at(iteration)
        assert position_rate_at(iteration) != position_rate_at(iteration + 1)
        s = scene_of(self)
        mom, steps = moments_of(self)
        calls, refines = self.refinement_calls, iteration in REFINEMENTS
        assert calls == len(log["refinements"]) == len(self.history)
        scale = MC.LOOP["noise_lr"] * position_rate_at(iteration)
        sc = self.scene
        clone = SimpleNamespace(point_cloud=sc.point_cloud.detach().clone(), point_cloud_features=sc.point_cloud_features.detach().clone(),
                                point_invalid_mask=sc.point_invalid_mask.clone(), point_object_id=sc.point_object_id.clone())
        mcmc.inject_noise(clone, scale, iteration, seed=MC.LOOP["seed"])
        if refines:
            for name in ("source_of", "dest_row", "multiplicity"):
                getattr(self.plan, name).fill_(-7)                  # what the call does not write stays (check_relocate)
        original["after"](self, iteration, position_lr)
        # the noise, on the clone: against float64 from the state before the call
        noised = dict(s, pc=host(clone.point_cloud))
        delta, magnitude, moves, smallest = mcmc_ref.noise(s["ft"], s["mask"], scale, MC.LOOP["seed"], iteration, with_smallest_term=True)
        assert np.array_equal(bits(noised["pc"][~moves]), bits(s["pc"][~moves]))
        normal = moves & (smallest >= SMALLEST_NORMAL)
        err = np.abs(noised["pc"].astype(np.float64) - (s["pc"].astype(np.float64) + delta))
        half = 0.5 * ulp32(noised["pc"])
        assert (err[normal] <= 2e-5 * magnitude[normal] + half[normal]).all()
        assert (np.abs(noised["pc"].astype(np.float64) - s["pc"]) <= 1.001 * magnitude + half + 1e-44).all()
        moved = (np.abs(delta) > ulp32(s["pc"])).any(1) & normal
        assert moved.sum() >= 10 and (bits(noised["pc"])[moved] != bits(s["pc"])[moved]).any(1).all(), int(moved.sum())
        assert_same_bits(dict(ft=host(clone.point_cloud_features), mask=host(clone.point_invalid_mask), obj=host(clone.point_object_id)),
                         {k: s[k] for k in ("ft", "mask", "obj")}, "noise")
        log["after"].append(int(moved.sum()))
        if not refines:
            assert_same_bits(scene_of(self), noised, "after_step without a refinement")
            assert_moments_kept(self, mom, steps, "after_step without a refinement")
            assert self.refinement_calls == calls and len(self.history) == calls
            return
        # the relocation, from the noised scene
        ref = mcmc_ref.relocate(noised["pc"], noised["ft"], noised["mask"], noised["obj"], MC.LOOP["seed"], calls)
        assert self.refinement_calls == calls + 1 and len(self.history) == calls + 1 and self.history[-1][0] == iteration
        after, (after_moments, after_steps) = scene_of(self), moments_of(self)
        got = dict(after, counts=[int(x) for x in self.history[-1][1].cpu()], dest_row=host(self.plan.dest_row), source_of=host(self.plan.source_of),
                   multiplicity=host(self.plan.multiplicity), moments=after_moments)
        assert np.array_equal(host(self.plan.counts), host(self.history[-1][1])) and after_steps == steps
        check_relocate(noised, got, ref, mom)
        c = dict(zip(mcmc_ref.COUNTS, ref["counts"]))
        assert (c["dead"] > 0 or calls > 0) and c["new"] == c["valid_before"] * 50 // 1000 > 0 and c["sources"] > 0     # dead rows at the first
        assert any(m.any() for m in mom) and ref["touched"].sum() > c["destinations"]
        D = c["destinations"]
        for other in {0, 1, 2, iteration} - {calls}:                # the call index decides the draw
            assert mcmc_ref.draw_sources(ref["weights"], D, MC.LOOP["seed"], other)[0] != ref["source_of"], other
        log["refinements"].append((iteration, c, ref["source_of"]))

    monkeypatch.setattr(FusedAdam, "step", step)
    monkeypatch.setattr(MCMCStrategy, "before_step", before_step)
    monkeypatch.setattr(MCMCStrategy, "after_step", after_step)
    trainer.train()
    assert len(log["before"]) == len(log["after"]) == ITERATIONS
    assert [it for it, _, _ in log["refinements"]] == REFINEMENTS and trainer.mcmc.refinement_calls == 3
    sources = [tuple(source_of) for _, _, source_of in log["refinements"]]
    assert len(set(sources)) == 3
    for it, c, _ in log["refinements"]:
        print(f"iteration {it}: " + " / ".join(str(c[k]) for k in mcmc_ref.COUNTS[:7]) + f" -> {c['valid_after']}")
    print("rows moved by more than an ulp, per iteration:", log["after"])
    print(f"regulariser in the loop: worst use of the bound {max(log['before']):.3g}")
