"""GPU: adaptive density control inside the training iteration -- the rasteriser's backward hook, the select in it, FusedAdam's
step, then the apply -- against density_ref.ReferenceController, on the inputs that tests/test_density_loop_ref_host.py fixes
(density_loop_case.py: 3000 points in 4500 rows at 64x48, three poses, 14 iterations, six densifications, two alpha resets).

The comparison is teacher-forced, one step at a time.  At the hook the reference gets copies of the payload and of the scene as
it is then, and its update() is compared with the device's: accumulators, and on densify iterations the plan.  After the
optimiser's step the reference applies its own densify info, with its own call index, to a copy of the device's stepped scene,
and the two scenes are compared.  Then the device's scene and accumulators replace the reference's, so that every comparison
tests one step and none carries the rounding of an earlier one.

What is exact: the integer accumulators; the view-space sums (one IEEE add per row and frame, for the average one IEEE divide
before it); the position-gradient sums (one add per component); the plan (flags, ids, snapshots, gradient positions, factors,
counts); after the apply the mask, the object ids, every feature (column 7 after a reset among them), the fill rows, and the
positions of every row that GaussianPoint3D.sample() did not draw.  Sampled positions: the 1e-5 of test_gpu_density.py.

accumulated_position_gradients_norm is compared bit for bit where the orders agree and otherwise within norm_bound().  Both sides
start a frame from the same value A >= 0 of a row (the device's, see above) and add the norm n of the same three f32 numbers.
With u = 2^-24: each square is one rounding, the two additions of positive terms one each, so the sum of squares is within
(1+u)^3 - 1 < 3.01 u of the exact one whatever the order or the contraction into fused multiply-adds; the square root halves
that and rounds once: |n' - n| <= 2.51 u n on either side, 5.02 u n between them.  The final add rounds once per side:
|fl(A + n1) - fl(A + n2)| <= |n1 - n2| + 2 u (A + n) (1 + 6 u).  With n <= A + n = the reference's new value `want` that is
less than 8 u want.  A square below 2^-126 loses at most 2^-126 absolutely (all of it, if subnormals are flushed), three of
them 3 * 2^-126 under the root, which moves the root by at most sqrt(3) * 2^-63 < 2^-62 per side.  norm_bound = 8 u want +
2^-61: 4.8e-7 relative, against the 1e-4 of the largest value (parity_util.GRAD_TOL) that
test_controller_accumulators_match_reference_update allows, and the test asserts that it is nowhere wider than that.
Measured on an MI355X: over a run some 3700 of the 14 x 4500 compared values differ in bits (the two sides do not form the sum of
squares alike), the worst of them at 0.40 of the bound.

The device's counts on an MI355X, hook wiring with the dense step (densify / fillable / over / under / transparent / floaters,
valid before -> after): iteration 2: 2095 / 2095 / 1048 / 1047 / 774 / 0, 3000 -> 4321; 4: 3733 / 190 / 13 / 177 / 11 / 0,
4321 -> 4500; 6: 3770 / 44 / 0 / 44 / 18 / 26, 4500 -> 4500; 8: 3686 / 15 / 0 / 15 / 10 / 5; 10: 3697 / 13 / 0 / 13 / 9 / 4;
12: 3697 / 9 / 0 / 9 / 6 / 3, the scene full from iteration 4 on.  With the rasteriser accumulating and the row-selective step:
2: the same; 4: 3737 / 189 / 13 / 176 / 10 / 0; 6: 3780 / 42 / 0 / 42 / 16 / 26; 8: 3690 / 15 / 0 / 15 / 10 / 5;
10: 3707 / 12 / 0 / 12 / 8 / 4; 12: 3717 / 9 / 0 / 9 / 6 / 3; 97 % of the first cycle's under-reconstructed sources had moved
(the others are rows the selecting frame did not touch).

A library whose k_density_fill gives the clone the source's current position instead of the plan's snapshot passes every test
of test_gpu_density.py and fails both cases here at iteration 2, on the positions of the rows that were not sampled."""
import numpy as np
import pytest
import torch

import density_loop_case as L
import parity_util
from density_ref import ACCUMULATORS, ReferenceController
from test_gpu_density import assert_apply_matches, assert_plan_matches

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
U = 2.0 ** -24
EXACT = [name for name, _, _ in ACCUMULATORS if name != "accumulated_position_gradients_norm"]


def norm_bound(want):
    return 8 * U * np.abs(want).astype(np.float64) + 2.0 ** -61


def _cpu(ctl):
    mp = ctl.maintained_parameters
    return [t.detach().cpu().clone() for t in (mp.pointcloud, mp.pointcloud_features, mp.point_invalid_mask, mp.point_object_id)]


def _device_accumulators(ctl):
    return {name: getattr(ctl.accumulators, name).cpu().clone() for name, _, _ in ACCUMULATORS}


def _bits(x):
    return x.numpy().view(np.int32)


def run_loop(rasteriser_accumulates):
    """-> (cycle records of the device, alpha resets, share of moved sources in the first cycle, worst use of norm_bound())"""
    from taichi_3d_gaussian_splatting_amd import CameraInfo, GaussianPointAdaptiveController as Ctl, GaussianPointCloudRasterisation as Rast
    from taichi_3d_gaussian_splatting_amd.optim import FusedAdam
    pc, ft, mask, obj, s = L.scene_arrays()
    pc = torch.tensor(pc, device=DEV, requires_grad=True)
    ft = torch.tensor(ft, device=DEV, requires_grad=True)
    mask, obj = torch.tensor(mask, device=DEV), torch.tensor(obj, device=DEV)
    cfg = L.controller_config()
    ctl = Ctl(cfg, Ctl.GaussianPointAdaptiveControllerMaintainedParameters(pc, ft, mask, obj), seed=L.SAMPLE_SEED,
              rasteriser_accumulates=rasteriser_accumulates)
    ref = ReferenceController(cfg, *_cpu(ctl), seed=L.SAMPLE_SEED)
    state = dict(info=None, hooks=0, norm_use=0.0, norm_bits_differ=0)

    def hook(payload):
        """the reference's update() on copies, the device's update(), and the two compared"""
        state["hooks"] += 1
        ref.pc, ref.feat, ref.mask, ref.obj = _cpu(ctl)
        cpu_payload = L.payload_of(*[t.cpu().clone() for t in (payload.point_id_in_camera_list, payload.num_affected_pixels,
                                                               payload.magnitude_grad_viewspace, payload.point_depth,
                                                               payload.grad_point_in_camera)])
        info = ref.update(cpu_payload)
        ctl.update(payload)
        assert ctl.iteration_counter == ref.iteration_counter
        got = _device_accumulators(ctl)
        for name in EXACT:
            assert got[name].dtype == ref.acc[name].dtype and torch.equal(got[name], ref.acc[name]), name
        a, want = got["accumulated_position_gradients_norm"].numpy(), ref.acc["accumulated_position_gradients_norm"].numpy()
        bound = norm_bound(want)
        err = np.abs(a.astype(np.float64) - want.astype(np.float64))
        assert np.all(err <= bound), float((err / bound).max())
        assert bound.max() <= parity_util.GRAD_TOL * np.abs(want).max()
        assert np.abs(want).max() > 0 and ref.acc["accumulated_num_in_camera"].sum() > 0
        state["norm_use"] = max(state["norm_use"], float((err / bound).max()))
        state["norm_bits_differ"] += int((_bits(torch.from_numpy(a)) != _bits(torch.from_numpy(want))).sum())
        if info is not None:
            plan = {k: (v.cpu().clone() if isinstance(v, torch.Tensor) else v) for k, v in ctl.densify_plan().items()}
            assert_plan_matches(plan, info)
            c = plan["counts"]
            assert (c["densify"], c["floaters"], c["transparent"]) == (
                info["densify_point_id"].shape[0], int(info["floater_mask"].sum()), int(info["transparent_mask"].sum()))
            assert c["single_frame"] == info["num_to_densify"] and c["single_frame_viewspace"] == info["num_to_densify_by_viewspace"]
        state["info"] = info
        ref.acc = got                                                     # the device's accumulators replace the reference's

    module = Rast(Rast.GaussianPointCloudRasterisationConfig(), backward_valid_point_hook=hook,
                  controller_accumulators=ctl.accumulators if rasteriser_accumulates else None)
    module.track_touched_rows = rasteriser_accumulates
    opt = FusedAdam([pc, ft], lr=L.LEARNING_RATE)
    cam = CameraInfo(torch.tensor(s.camera_intrinsics, device=DEV), s.height, s.width, 0)
    gt = torch.full((s.height, s.width, 3), L.TARGET, device=DEV)
    cycles, resets, moved_share = [], [], None
    for it in range(L.N_ITERATIONS):
        q, t = L.pose(it)
        opt.zero_grad()
        img, _, _ = module(Rast.GaussianPointCloudRasterisationInput(pc, ft, obj, mask, cam, torch.tensor(q, device=DEV),
                                                                      torch.tensor(t, device=DEV), color_max_sh_band=L.BAND))
        ((img - gt) ** 2).sum().backward()
        assert state["hooks"] == it + 1
        info = state["info"]
        assert (info is not None) == L.ctl_densifies(cfg, it)
        if rasteriser_accumulates:
            opt.step(rows=module.last_touched_rows)
        else:
            opt.step()
        ref.pc, ref.feat, ref.mask, ref.obj = _cpu(ctl)                    # the stepped scene, before either side refines it
        done = ref.refinement()
        ctl.refinement()
        got_pc, got_feat, got_mask, got_obj = _cpu(ctl)
        assert (done is None) == (it < cfg.num_iterations_warm_up)
        if done is not None and done["counts"] is not None:
            counts = ctl.last_refinement_counts()
            fill = ctl.densify_plan()["fill_point_id"].cpu().numpy()
            got = dict(pc=got_pc.numpy(), feat=got_feat.numpy(), mask=got_mask.numpy(), obj=got_obj.numpy(), fill=fill)
            want = dict(pc=ref.pc.numpy(), feat=ref.feat.numpy(), mask=ref.mask.numpy(), obj=ref.obj.numpy())
            assert_apply_matches(got, counts, want, done["counts"], info, cfg)
            assert ctl.refinement_calls == ref.refinement_calls == len(cycles) + 1
            for name, acc in _device_accumulators(ctl).items():
                assert not acc.any(), name                                  # reset by refinement()
            flags = ctl.densify_plan()["flags"].cpu().numpy()
            device_info = dict(floater_mask=(flags & 1) != 0, transparent_mask=(flags & 2) != 0)
            cycles.append(L.cycle_record(it, dict(counts, fill_point_id=fill), device_info, pc.shape[0]))
            if moved_share is None:
                plan = {k: v.cpu() for k, v in ctl.densify_plan().items() if isinstance(v, torch.Tensor)}
                plan["densify_size_reduction_factor"] = plan["densify_size_reduction_factor"][:, None]
                moved_share = L.moved_sources_share(counts, plan, got_pc.numpy())
        else:                                                               # no apply: at most the alpha reset touched the scene
            assert np.array_equal(_bits(got_pc), _bits(ref.pc)) and np.array_equal(_bits(got_feat), _bits(ref.feat))
            assert torch.equal(got_mask, ref.mask) and torch.equal(got_obj, ref.obj)
        if done is not None and done["reset_alpha"]:
            assert np.array_equal(_bits(got_feat[:, 7]), _bits(ref.feat[:, 7])) and float(got_feat[:, 7].max()) <= cfg.reset_alpha_value
            resets.append((it, done["counts"] is not None, done["rows_lowered"]))
        ref.pc, ref.feat, ref.mask, ref.obj = got_pc, got_feat, got_mask, got_obj
        ref.acc = _device_accumulators(ctl)
        print(f"iteration {it}: compared" + (f", cycle {len(cycles)}" if done is not None and done["counts"] is not None else ""))
    return cycles, resets, moved_share, state


@pytest.mark.parametrize("rasteriser_accumulates", [False, True], ids=["hook_wiring_dense_adam", "rasteriser_accumulates_row_adam"])
def test_device_loop_matches_the_reference_step_by_step(rasteriser_accumulates):
    cycles, resets, moved_share, state = run_loop(rasteriser_accumulates)
    print(L.counts_table(cycles))
    print("alpha resets (iteration, on a densify iteration, rows lowered):", resets, " moved sources:", moved_share)
    print(f"norm accumulator: {state['norm_bits_differ']} values differ in bits, worst use of the bound {state['norm_use']:.3g}")
    assert [c["iteration"] for c in cycles] == [2, 4, 6, 8, 10, 12]
    assert [r[:2] for r in resets] == [(5, False), (10, True)]
    assert all(rows_lowered >= 100 for _, _, rows_lowered in resets)
    L.assert_branch_conditions(cycles, resets, moved_share, L.controller_config())
