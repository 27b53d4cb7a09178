"""GPU: adaptive density control on the device (gs_density_select / gs_density_apply / gs_controller_accumulate and
GaussianPointAdaptiveController) against the line-by-line restatement of the reference controller in density_ref.py
(CTRL = taichi_3d_gaussian_splatting/GaussianPointAdaptiveController.py), run on the CPU."""
import types

import numpy as np
import pytest
import torch

from density_ref import add_densify_points, find_densify_points, rotation_matrix

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ACC_NAMES = ["accumulated_num_in_camera", "accumulated_num_pixels", "accumulated_view_space_position_gradients",
             "accumulated_view_space_position_gradients_avg", "accumulated_position_gradients", "accumulated_position_gradients_norm"]


def _ctl_cls():
    from taichi_3d_gaussian_splatting_amd import GaussianPointAdaptiveController
    return GaussianPointAdaptiveController


def make_case(N=5000, n_valid=3000, M=1500, seed=0, nan_rows=(7, 1234)):
    """A pre-allocated scene (first n_valid rows valid, a few free rows among them), accumulators and a hook payload with
    every branch of CTRL:170-265 represented."""
    rng = np.random.default_rng(seed)
    pc = rng.normal(0, 1, (N, 3)).astype(np.float32)
    feat = rng.normal(0, 1, (N, 56)).astype(np.float32)
    feat[:, 4:7] = rng.uniform(-4, -1, (N, 3)).astype(np.float32)
    feat[:, 7] = rng.uniform(-0.8, 2.0, N).astype(np.float32)              # alpha logit: some below -0.5 (transparent)
    mask = np.ones(N, np.int8)
    mask[:n_valid] = 0
    mask[rng.choice(n_valid, n_valid // 20, replace=False)] = 1            # free rows among the valid ones
    for r in nan_rows:
        feat[r, 30] = np.nan                                                # a NaN in an SH column of a valid row
        mask[r] = 0
    pc[mask == 1] = 0
    obj = rng.integers(0, 4, N).astype(np.int32)
    valid_ids = np.flatnonzero(mask == 0)
    ids = np.sort(rng.choice(valid_ids, min(M, valid_ids.size), replace=False)).astype(np.int32)
    M = ids.size
    npix = rng.integers(0, 20000, M).astype(np.int32)
    npix[rng.random(M) < 0.1] = 0
    depth = rng.uniform(0.5, 200, M).astype(np.float32)
    mag = rng.exponential(1e-5, M).astype(np.float32)
    mag[rng.random(M) < 0.1] = 0
    nic = rng.integers(0, 6, N).astype(np.int32)
    nic[mask == 1] = 0
    acc = dict(accumulated_num_in_camera=nic,
               accumulated_num_pixels=(nic * rng.integers(0, 3000, N)).astype(np.int32),
               accumulated_view_space_position_gradients=(nic * rng.exponential(1e-5, N)).astype(np.float32),
               accumulated_view_space_position_gradients_avg=(nic * rng.exponential(1e-8, N)).astype(np.float32),
               accumulated_position_gradients=(nic[:, None] * rng.normal(0, 1e-3, (N, 3))).astype(np.float32),
               accumulated_position_gradients_norm=(nic * rng.exponential(1e-3, N)).astype(np.float32))
    scene = dict(pc=pc, feat=feat, mask=mask, obj=obj)
    hook = dict(ids=ids, npix=npix, depth=depth, mag=mag)
    return scene, acc, hook


def low_config(many=True, **kw):
    Ctl = _ctl_cls()
    base = dict(num_iterations_warm_up=0, num_iterations_densify=1, iteration_start_remove_floater=0,
                transparent_alpha_threshold=-0.5,
                densification_view_space_position_gradients_threshold=2e-5 if many else 6e-5,
                densification_view_avg_space_position_gradients_threshold=2e-9 if many else 1e-8,
                densification_multi_frame_view_space_position_gradients_threshold=2e-5 if many else 1e-4,
                densification_multi_frame_view_pixel_avg_space_position_gradients_threshold=5e-12 if many else 1e-10,
                densification_multi_frame_position_gradients_threshold=3e-3 if many else 1e-2,
                floater_near_camrea_num_pixels_threshold=15000, floater_depth_threshold=100.0,
                under_reconstructed_num_pixels_threshold=2500, under_reconstructed_move_factor=100.0)
    base.update(kw)
    return Ctl.GaussianPointAdaptiveControllerConfig(**base)


def build_controller(scene, acc, cfg, seed=0):
    Ctl = _ctl_cls()
    t = {k: torch.tensor(v, device=DEV) for k, v in scene.items()}
    ctl = Ctl(cfg, Ctl.GaussianPointAdaptiveControllerMaintainedParameters(
        pointcloud=t["pc"], pointcloud_features=t["feat"], point_invalid_mask=t["mask"], point_object_id=t["obj"]), seed=seed)
    for k, v in acc.items():
        getattr(ctl.accumulators, k).copy_(torch.tensor(v, device=DEV))
    return ctl


def hook_payload(hook):
    t = {k: torch.tensor(v, device=DEV) for k, v in hook.items()}
    return types.SimpleNamespace(point_id_in_camera_list=t["ids"], num_affected_pixels=t["npix"], point_depth=t["depth"],
                                 magnitude_grad_viewspace=t["mag"])


def run_device(scene, acc, hook, cfg, seed=0, remove_floaters=True):
    ctl = build_controller(scene, acc, cfg, seed)
    ctl.iteration_counter = 1 if remove_floaters else -1
    ctl.config.iteration_start_remove_floater = 0
    ctl._find_densify_points(hook_payload(hook))
    plan = {k: (v.cpu().clone() if isinstance(v, torch.Tensor) else v) for k, v in ctl.densify_plan().items()}
    ctl._add_densify_points()
    torch.cuda.synchronize()
    mp = ctl.maintained_parameters
    out = dict(pc=mp.pointcloud.cpu().numpy(), feat=mp.pointcloud_features.cpu().numpy(), mask=mp.point_invalid_mask.cpu().numpy(),
               obj=mp.point_object_id.cpu().numpy(), fill=ctl.densify_plan()["fill_point_id"].cpu().numpy())
    return plan, out, ctl.last_refinement_counts()


def run_reference(scene, acc, hook, cfg, seed=0, call_index=0, remove_floaters=True):
    t = {k: torch.tensor(v) for k, v in scene.items()}
    a = {k: torch.tensor(v) for k, v in acc.items()}
    h = {k: torch.tensor(v) for k, v in hook.items()}
    info = find_densify_points(t["pc"], t["feat"], t["mask"], a, h["ids"], h["npix"], h["depth"], h["mag"], remove_floaters, cfg)
    counts = add_densify_points(t["pc"], t["feat"], t["mask"], t["obj"], info, cfg, seed, call_index)
    return info, {k: v.numpy() for k, v in t.items()}, counts


def assert_plan_matches(plan, info):
    """a select's plan (densify_plan(), on the CPU) against find_densify_points' info: masks, ids, snapshots, factors, bit for bit"""
    flags = plan["flags"].numpy().astype(np.int64)
    assert np.array_equal((flags & 1) != 0, info["floater_mask"].numpy())
    assert np.array_equal((flags & 2) != 0, info["transparent_mask"].numpy())
    assert np.array_equal((flags & 4) != 0, info["densify_mask"].numpy())
    assert np.array_equal(plan["densify_point_id"].numpy(), info["densify_point_id"].numpy())
    assert np.array_equal(plan["densify_point_position_before_optimization"].numpy(), info["densify_point_position_before_optimization"].numpy())
    assert np.array_equal(plan["densify_point_grad_position"].numpy(), info["densify_point_grad_position"].numpy())
    assert np.array_equal(plan["densify_size_reduction_factor"].numpy(), info["densify_size_reduction_factor"].numpy()[:, 0])


def assert_apply_matches(got, counts, want, ref_counts, info, cfg, pos_rtol=1e-5):
    """the scene after an apply (got: pc, feat, mask, obj, fill as numpy; counts: last_refinement_counts()) against
    add_densify_points' scene and counts"""
    assert np.array_equal(got["fill"], ref_counts["fill_point_id"].numpy())
    for k in ["floaters", "transparent", "densify", "fillable", "over", "under", "valid_before", "valid_after"]:
        assert counts[k] == ref_counts[k], (k, counts[k], ref_counts[k])
    assert counts["single_frame"] == info["num_to_densify"]
    assert counts["single_frame_viewspace"] == info["num_to_densify_by_viewspace"]
    # the scene after apply: masks, object ids, copied and reduced features bit for bit (NaN rows compared as NaN)
    assert np.array_equal(got["mask"], want["mask"]) and np.array_equal(got["obj"], want["obj"])
    assert np.array_equal(got["feat"], want["feat"], equal_nan=True)
    # positions: bit for bit except where GaussianPoint3D.sample() drew (f32 transcendental tolerance there)
    nf = counts["fillable"]
    d = info["densify_point_id"].numpy()[:nf]
    f = got["fill"]
    over = info["densify_size_reduction_factor"].numpy()[:nf, 0] > 1e-6
    sampled = np.zeros(len(got["pc"]), bool)
    if cfg.enable_sample_from_point:
        sampled[d[over]] = True
        sampled[f[over]] = True
    if not cfg.enable_ellipsoid_offset:
        assert np.array_equal(got["pc"][~sampled], want["pc"][~sampled])
    else:
        assert np.allclose(got["pc"], want["pc"], rtol=pos_rtol, atol=pos_rtol)
    err = np.abs(got["pc"][sampled] - want["pc"][sampled])
    assert np.all(err <= pos_rtol * (np.abs(want["pc"][sampled]) + 1.0)), float(err.max(initial=0))


def assert_same_as_reference(scene, acc, hook, cfg, seed=0, remove_floaters=True, pos_rtol=1e-5, call_index=0):
    """one select and one apply of a fresh controller against the reference's; call_index: of the reference's sample stream
    (a fresh controller's first apply draws from call 0)"""
    plan, got, counts = run_device(scene, acc, hook, cfg, seed, remove_floaters)
    info, want, ref_counts = run_reference(scene, acc, hook, cfg, seed, call_index, remove_floaters)
    assert_plan_matches(plan, info)
    assert_apply_matches(got, counts, want, ref_counts, info, cfg, pos_rtol)
    return counts, info


@pytest.mark.parametrize("many", [True, False], ids=["more_candidates_than_free_rows", "fewer_candidates"])
def test_select_apply_match_reference(many):
    scene, acc, hook = make_case(seed=1, n_valid=4800) if many else make_case(seed=2)
    cfg = low_config(many)
    counts, info = assert_same_as_reference(scene, acc, hook, cfg, seed=123)
    # every branch fired
    assert counts["floaters"] > 0 and counts["transparent"] > 0 and counts["over"] > 0 and counts["under"] > 0
    assert info["transparent_mask"].numpy()[[7, 1234]].all()             # the NaN rows
    assert counts["single_frame_viewspace"] > 0 and counts["single_frame"] > counts["single_frame_viewspace"]
    assert counts["densify"] > counts["single_frame"]                       # multi-frame criteria added rows
    n_free = int((scene["mask"] == 1).sum()) + counts["floaters"] + counts["transparent"]
    if many:
        assert counts["densify"] > n_free and counts["fillable"] == n_free  # truncation
    else:
        assert counts["densify"] < n_free and counts["fillable"] == counts["densify"]


def test_no_floater_removal_before_start():
    scene, acc, hook = make_case(seed=3)
    counts, _ = assert_same_as_reference(scene, acc, hook, low_config(True), remove_floaters=False)
    assert counts["floaters"] == 0


def test_ellipsoid_offset_matches_reference():
    """enable_ellipsoid_offset (CTRL:322-328, GP3D:376-388) including the base-axis choice of equal / middle scales."""
    scene, acc, hook = make_case(seed=4)
    rng = np.random.default_rng(4)
    feat = scene["feat"]
    feat[:, 0:4] /= np.linalg.norm(feat[:, 0:4], axis=1, keepdims=True)
    pattern = np.array([[-2, -2, -3], [-3, -2, -2], [-2, -3, -2], [-3, -2, -1], [-1, -2, -3], [-2, -2, -2]], np.float32)
    feat[:, 4:7] = pattern[rng.integers(0, len(pattern), len(feat))]
    cfg = low_config(True, enable_ellipsoid_offset=True, enable_sample_from_point=False)
    assert_same_as_reference(scene, acc, hook, cfg)
    cfg = low_config(True, enable_ellipsoid_offset=True, enable_sample_from_point=True)
    assert_same_as_reference(scene, acc, hook, cfg, pos_rtol=2e-5)


def test_split_samples_have_the_gaussian_distribution():
    """20 000 identical over-reconstructed points: clone and original samples ~ N(centre, R S^2 R^T) with the reduced S."""
    n = 20000
    N = 2 * n
    q = np.array([0.2, -0.4, 0.1, 0.9], np.float32)
    q /= np.linalg.norm(q)
    s = np.array([-1.0, -2.0, -1.5], np.float32)
    centre = np.array([0.5, -1.0, 2.0], np.float32)
    pc = np.zeros((N, 3), np.float32)
    pc[:n] = centre
    feat = np.zeros((N, 56), np.float32)
    feat[:n, 0:4] = q
    feat[:n, 4:7] = s
    feat[:n, 7] = 1.0
    mask = np.ones(N, np.int8)
    mask[:n] = 0
    scene = dict(pc=pc, feat=feat, mask=mask, obj=np.zeros(N, np.int32))
    acc = {k: np.zeros((N, 3) if k == "accumulated_position_gradients" else N, np.int32 if "num_" in k else np.float32) for k in ACC_NAMES}
    acc["accumulated_num_in_camera"][:n] = 1
    acc["accumulated_num_pixels"][:n] = 1000
    hook = dict(ids=np.arange(n, dtype=np.int32), npix=np.full(n, 1000, np.int32), depth=np.full(n, 5, np.float32),
                mag=np.full(n, 1.0, np.float32))
    cfg = low_config(True, under_reconstructed_num_pixels_threshold=512)
    plan, got, counts = run_device(scene, acc, hook, cfg, seed=99)
    assert counts["fillable"] == n and counts["over"] == n
    x = np.concatenate([got["pc"][:n], got["pc"][n:]]).astype(np.float64)
    s_red = s - np.float32(np.log(1.6))
    assert np.array_equal(got["feat"][:, 4:7], np.tile(s_red, (N, 1)))
    R = rotation_matrix(torch.tensor(q[None].astype(np.float64)))[0].numpy()
    cov = R @ np.diag(np.exp(2 * s_red.astype(np.float64))) @ R.T
    m = x.mean(0)
    sd = np.sqrt(np.diag(cov))
    assert np.all(np.abs(m - centre) < 4 * sd / np.sqrt(len(x))), (m, centre)
    emp = np.cov(x.T)
    assert np.abs(emp - cov).max() < 0.03 * np.abs(cov).max(), (emp, cov)
    d = x - centre
    md2 = np.einsum("ni,ij,nj->n", d, np.linalg.inv(cov), d)
    assert abs(md2.mean() - 3.0) < 4 * np.sqrt(6.0 / len(x))               # chi^2(3): mean 3, variance 6
    assert abs(md2.var() - 6.0) < 0.3
    assert abs(np.mean(md2 < 2.3660) - 0.5) < 0.01                          # its median


def _three_refinements(seed):
    scene, acc, hook = make_case(seed=6)
    cfg = low_config(False)
    ctl = build_controller(scene, acc, cfg, seed)
    ctl.iteration_counter = 1
    for _ in range(3):
        ctl._find_densify_points(hook_payload(hook))
        ctl._add_densify_points()
    torch.cuda.synchronize()
    mp = ctl.maintained_parameters
    return ctl, [t.cpu().numpy() for t in (mp.pointcloud, mp.pointcloud_features, mp.point_invalid_mask, mp.point_object_id)]


def test_same_seed_is_bit_identical_and_seed_changes_only_samples():
    ctl_a, a = _three_refinements(7)
    _, b = _three_refinements(7)
    _, c = _three_refinements(8)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)
    assert np.array_equal(a[1], c[1], equal_nan=True) and np.array_equal(a[2], c[2]) and np.array_equal(a[3], c[3])
    differ = np.any(a[0] != c[0], axis=1)
    assert differ.any()
    assert ctl_a.refinement_calls == 3
    # exactly the rows that were split in some call differ; that set is a subset of the rows changed by densification
    scene, _, _ = make_case(seed=6)
    moved = np.any(a[0] != scene["pc"], axis=1)
    assert not (differ & ~moved).any()


def _render_setup(seed):
    from taichi_3d_gaussian_splatting_amd.scene_io import preallocate
    from taichi_3d_gaussian_splatting_amd.synthetic import synth, view_pose
    s = synth(3000, 64, 48, 0.08, sh_deg=3, seed=seed)
    pc, ft, mask, obj = preallocate(s.point_cloud, s.point_cloud_features, 1.5)
    q, t = view_pose(0, 1)
    return pc, ft, mask, obj, s, q, t


def _wired_run(rasteriser_accumulates, iters=3):
    from taichi_3d_gaussian_splatting_amd import CameraInfo, GaussianPointCloudRasterisation as Rast
    from taichi_3d_gaussian_splatting_amd.optim import FusedAdam
    Ctl = _ctl_cls()
    pc, ft, mask, obj, s, q, t = _render_setup(11)
    pc = torch.tensor(pc, device=DEV, requires_grad=True)
    ft = torch.tensor(ft, device=DEV, requires_grad=True)
    mask, obj = torch.tensor(mask, device=DEV), torch.tensor(obj, device=DEV)
    cfg = Ctl.GaussianPointAdaptiveControllerConfig(num_iterations_warm_up=2, num_iterations_densify=2,
                                                    densification_view_space_position_gradients_threshold=0.0,
                                                    under_reconstructed_num_pixels_threshold=50)
    ctl = Ctl(cfg, Ctl.GaussianPointAdaptiveControllerMaintainedParameters(pc, ft, mask, obj), seed=5,
              rasteriser_accumulates=rasteriser_accumulates)
    module = Rast(Rast.GaussianPointCloudRasterisationConfig(), backward_valid_point_hook=ctl.update,
                  controller_accumulators=ctl.accumulators if rasteriser_accumulates else None)
    opt = FusedAdam([pc, ft], lr=1e-3)
    cam = CameraInfo(torch.tensor(s.camera_intrinsics, device=DEV), s.height, s.width, 0)
    qd, td = torch.tensor(q, device=DEV), torch.tensor(t, device=DEV)
    gt = torch.full((s.height, s.width, 3), 0.3, device=DEV)
    acc_before_refinement = None
    for i in range(iters):
        opt.zero_grad()
        img, _, _ = module(Rast.GaussianPointCloudRasterisationInput(pc, ft, obj, mask, cam, qd, td, color_max_sh_band=3))
        ((img - gt) ** 2).sum().backward()
        opt.step()
        if i == iters - 1:
            acc_before_refinement = [getattr(ctl.accumulators, k).clone() for k in ACC_NAMES]
        ctl.refinement()
    torch.cuda.synchronize()
    return ctl, acc_before_refinement, [x.detach().cpu().numpy() for x in (pc, ft, mask, obj)]


def test_hook_and_rasteriser_accumulation_are_the_same():
    ctl_h, acc_h, scene_h = _wired_run(False)
    ctl_r, acc_r, scene_r = _wired_run(True)
    for name, x, y in zip(ACC_NAMES, acc_h, acc_r):
        assert torch.equal(x, y), name
        assert x.abs().sum() > 0, name
    assert ctl_h.last_refinement_counts() == ctl_r.last_refinement_counts()
    assert ctl_h.last_refinement_counts()["fillable"] > 0
    for x, y in zip(scene_h, scene_r):
        assert np.array_equal(x, y, equal_nan=True)
    assert ctl_r.accumulators.accumulated_num_in_camera.sum() == 0       # reset by refinement(), in place


def test_edges():
    cfg = low_config(True)
    # M = 0: only the N-pass criteria (transparent, multi-frame)
    scene, acc, hook = make_case(seed=8)
    empty = {k: v[:0] for k, v in hook.items()}
    counts, _ = assert_same_as_reference(scene, acc, empty, cfg)
    assert counts["floaters"] == 0 and counts["single_frame"] == 0 and counts["densify"] > 0
    # no candidates at all (infinite thresholds: x/0 -> inf passes any finite one, as in torch)
    none = low_config(True, transparent_alpha_threshold=-np.inf, **{k: np.inf for k in [
        "densification_view_space_position_gradients_threshold", "densification_view_avg_space_position_gradients_threshold",
        "densification_multi_frame_view_space_position_gradients_threshold",
        "densification_multi_frame_view_pixel_avg_space_position_gradients_threshold",
        "densification_multi_frame_position_gradients_threshold"]}, floater_near_camrea_num_pixels_threshold=2 ** 31 - 1)
    scene, acc, hook = make_case(seed=9, nan_rows=())
    counts, _ = assert_same_as_reference(scene, acc, hook, none)
    assert counts["densify"] == counts["fillable"] == counts["transparent"] == 0 and counts["valid_after"] == counts["valid_before"]
    # no free rows (every row valid), N not a multiple of the block size
    scene, acc, hook = make_case(N=1001, n_valid=1001, M=400, seed=10, nan_rows=())
    scene["mask"][:] = 0
    cfg_keep = low_config(True, transparent_alpha_threshold=-np.inf, floater_near_camrea_num_pixels_threshold=2 ** 31 - 1)
    counts, _ = assert_same_as_reference(scene, acc, hook, cfg_keep)
    assert counts["densify"] > 0 and counts["fillable"] == 0 and counts["valid_after"] == 1001
    # every row invalid
    scene, acc, hook = make_case(N=777, n_valid=0, M=0, seed=11, nan_rows=())
    counts, _ = assert_same_as_reference(scene, acc, hook, cfg)
    assert counts["valid_before"] == counts["valid_after"] == 0 and counts["densify"] == 0
    # N = 0
    scene, acc, hook = make_case(N=0, n_valid=0, M=0, seed=12, nan_rows=())
    plan, got, counts = run_device(scene, acc, hook, cfg)
    assert all(v == 0 for v in counts.values())


# ---- past the thresholds of the scan and the fill --------------------------------------------------------------------------
# k_density_scan: one workgroup of 1024 threads, ceil(nb / 1024) per-block counts per thread (nb = ceil(N / 256) blocks);
# k_density_fill: min(nb, 1024) blocks of 256 pairs that stride over the fillable pairs.  Every case above has nb <= 157.
SCAN_THREADS, ROWS_PER_BLOCK, FILL_BLOCKS = 1024, 256, 1024
ALL_MULTI_FRAME = dict(densification_multi_frame_view_space_position_gradients_threshold=-1.0)    # every valid row a candidate


def _scan_shape(N):
    nb = -(-N // ROWS_PER_BLOCK)
    return nb, -(-nb // SCAN_THREADS)


def test_scan_with_two_block_counts_per_thread():
    """1025 blocks, the last one of a single row: threads 0..511 sum two counts each, thread 512 one, the rest none"""
    N = SCAN_THREADS * ROWS_PER_BLOCK + 1
    scene, acc, hook = make_case(N=N, n_valid=200000, M=100000, seed=21)
    nb, per = _scan_shape(N)
    assert nb == 1025 > SCAN_THREADS and per == 2 and N % ROWS_PER_BLOCK == 1
    counts, _ = assert_same_as_reference(scene, acc, hook, low_config(True))
    print(counts)
    assert counts["densify"] == counts["fillable"] > 0 and counts["floaters"] > 0 and counts["transparent"] > 0
    assert counts["over"] > 0 and counts["under"] > 0


@pytest.mark.parametrize("n_valid,truncated", [(360000, False), (450000, True)], ids=["every_candidate_filled", "more_candidates_than_free_rows"])
def test_fill_past_one_trip_of_its_grid(n_valid, truncated):
    """2735 blocks (three counts per scan thread) and more than 1024 x 256 fillable pairs: the fill grid strides a second time.
    With 450 000 valid rows the candidates outnumber the free rows and the scene ends full."""
    N = 700000
    scene, acc, hook = make_case(N=N, n_valid=n_valid, M=150000, seed=21)
    nb, per = _scan_shape(N)
    assert nb == 2735 > SCAN_THREADS and per == 3
    counts, _ = assert_same_as_reference(scene, acc, hook, low_config(True, **ALL_MULTI_FRAME))
    print(counts)
    assert counts["fillable"] > FILL_BLOCKS * ROWS_PER_BLOCK, counts
    assert counts["floaters"] > 0 and counts["transparent"] > 0 and counts["over"] > 0 and counts["under"] > 0
    assert counts["over"] + counts["under"] == counts["fillable"]
    if truncated:
        assert counts["densify"] > counts["fillable"] and counts["valid_after"] == N
    else:
        assert counts["densify"] == counts["fillable"] and counts["valid_after"] < N


def test_reference_controller_test_basic():
    """T_CTRL:15-95 (GaussianPointAdaptiveControllerTest.test_basic) shortened: 32x32 image, 10 000 rows of which 1 000
    valid, the reference's wiring (backward_valid_point_hook=controller.update), FusedAdam, ~400 iterations."""
    from taichi_3d_gaussian_splatting_amd import CameraInfo, GaussianPointCloudRasterisation as Rast
    from taichi_3d_gaussian_splatting_amd.optim import FusedAdam
    Ctl = _ctl_cls()
    torch.manual_seed(0)
    image_size = (32, 32)
    num_points = 10000
    fake_image = torch.zeros(size=(image_size[0], image_size[1], 3), dtype=torch.float32, device=DEV)
    fake_image[:5, :2, 0] = 1.0
    fake_image[:5, :2, 1] = 0.7
    fake_image[8:24, 8:24, 0] = 0.5
    fake_image[8:24, 8:24, 1] = 0.7
    fake_image[20:28, 20:28, 0] = 0.8
    fake_image[20:28, 20:28, 1] = 0.1
    point_cloud = torch.nn.Parameter((torch.rand(size=(num_points, 3), dtype=torch.float32, device=DEV) - 0.5) * 3)
    point_invalid_mask = torch.zeros((num_points,), dtype=torch.int8, device=DEV)
    point_invalid_mask[1000:] = 1
    tmp = torch.rand(size=(num_points, 56), dtype=torch.float32, device=DEV)
    tmp[:, 4:7] = -4.60517018599
    tmp[:, 7] = 0.5
    point_cloud_features = torch.nn.Parameter(tmp)
    point_object_id = torch.zeros((num_points,), dtype=torch.int32, device=DEV)
    camera_info = CameraInfo(camera_height=image_size[0], camera_width=image_size[1], camera_id=0,
                             camera_intrinsics=torch.tensor([[32, 0, 16], [0, 32, 16], [0, 0, 1]], dtype=torch.float32, device=DEV))
    q_camera_world = torch.tensor([0, 0, 0, 1], dtype=torch.float32, device=DEV).unsqueeze(0)
    t_camera_world = torch.tensor([0, 0, -2], dtype=torch.float32, device=DEV).unsqueeze(0)
    controller = Ctl(config=Ctl.GaussianPointAdaptiveControllerConfig(num_iterations_warm_up=100, num_iterations_densify=50,
                                                                      iteration_start_remove_floater=200, num_iterations_reset_alpha=300),
                     maintained_parameters=Ctl.GaussianPointAdaptiveControllerMaintainedParameters(
                         pointcloud=point_cloud, pointcloud_features=point_cloud_features,
                         point_invalid_mask=point_invalid_mask, point_object_id=point_object_id), seed=1)
    rast = Rast(config=Rast.GaussianPointCloudRasterisationConfig(near_plane=1., far_plane=10.),
                backward_valid_point_hook=controller.update)
    optimizer = FusedAdam([point_cloud, point_cloud_features], lr=0.001)
    initial_loss = latest_loss = None
    densified = 0
    for idx in range(400):
        optimizer.zero_grad()
        pred_image, _, _ = rast(Rast.GaussianPointCloudRasterisationInput(
            point_cloud=point_cloud, point_cloud_features=point_cloud_features, point_object_id=point_object_id,
            point_invalid_mask=point_invalid_mask, camera_info=camera_info, q_pointcloud_camera=q_camera_world,
            t_pointcloud_camera=t_camera_world, color_max_sh_band=min(idx // 100, 3)))
        loss = ((pred_image - fake_image) ** 2).sum()
        loss.backward()
        optimizer.step()
        valid_before = int((point_invalid_mask == 0).sum())
        controller.refinement()
        if idx >= 100 and idx % 50 == 0:
            c = controller.last_refinement_counts()
            valid_after = int((point_invalid_mask == 0).sum())
            assert c["valid_before"] == valid_before and c["valid_after"] == valid_after, (idx, c, valid_before, valid_after)
            assert valid_after == valid_before - c["floaters"] - c["transparent"] + c["fillable"]
            densified += c["fillable"]
            valid = point_invalid_mask == 0
            assert not torch.isnan(point_cloud[valid]).any() and not torch.isnan(point_cloud_features[valid]).any(), idx
        if idx == 0:
            initial_loss = loss.item()
        latest_loss = loss.item()
    assert controller.refinement_calls == 6 and densified > 0
    assert latest_loss < initial_loss
