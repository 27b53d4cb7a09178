"""GPU (-m gpu): the 3D smoothing filter (include/gs_filter3d.h, filter3d.py) against tests/filter3d_ref.py: the sampling rate
bit for bit over the shapes where the kernel changes path (a tail block, one row, no row; no view, one, two, seventeen) and
the comparisons' edges; the transform's pass-through columns and identity rows bit for bit and its float64 columns within one
float32 ulp; the gradient within one ulp of the float64 value; and through the rasteriser at 64x96."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import filter3d_ref as ref
import trainer_util as TU
from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast, filter3d
from taichi_3d_gaussian_splatting_amd.Camera import CameraInfo
from taichi_3d_gaussian_splatting_amd.filter3d import Filter3D, Filter3DConfig
from taichi_3d_gaussian_splatting_amd.synthetic import view_pose

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
W, H, NEAR, MARGIN = 96, 64, 0.8, 0.15
ROWS = [700, 1, 0]                      # three blocks of 256 with a tail of 188; one row; the empty scene
VIEWS = [0, 1, 2, 17]
FX0, FY0 = 64.0, 80.0                   # view 0: the identity pose, fx a power of two and cx = 0, so u = 64 x / z exactly
EDGE_ROWS = 12                          # the rows of rate_points() whose outcome under view 0 alone is asserted


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F)).view(np.int32)


def dev(a, **kw):
    return torch.tensor(np.asarray(a), device=DEV, **kw)


def view_rows(n_views):
    """view 0: the identity pose; the others: turned about y and x and moved, every fx != fy"""
    rng = np.random.default_rng(11)
    rows = [np.concatenate([np.eye(3).reshape(9), np.zeros(3), [FX0, FY0, 0.0, H / 2]])]
    for i in range(1, n_views):
        a, b = np.deg2rad(rng.uniform(-25, 25)), np.deg2rad(rng.uniform(-10, 10))
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        rows.append(np.concatenate([(Rx @ Ry).reshape(9), rng.uniform(-0.5, 0.5, 3),
                                    [rng.uniform(50, 90), rng.uniform(50, 90), W / 2 + rng.uniform(-3, 3), H / 2 + rng.uniform(-3, 3)]]))
    return np.asarray(rows[:n_views], dtype=F).reshape(-1, 16)


def rate_points(n):
    """(point_cloud, mask): the edge rows first, then a cloud around the cameras' frusta of which a part lies behind them and
    a part far outside, with invalid rows"""
    rng = np.random.default_rng(5)
    lo_x, hi_x, lo_y, hi_y = ref.window(W, H, MARGIN)
    up, down = lambda v: np.nextafter(F(v), F(np.inf)), lambda v: np.nextafter(F(v), F(-np.inf))
    edge = np.array([
        [0.0, 0.0, NEAR],                       # 0 exactly on the near plane: not beyond it
        [0.0, 0.0, up(NEAR)],                   # 1 the next float: seen
        [hi_x / F(FX0), 0.0, 1.0],              # 2 u == hi_x: seen
        [up(hi_x / F(FX0)), 0.0, 1.0],          # 3 one ulp outside
        [lo_x / F(FX0), 0.0, 1.0],              # 4 u == lo_x: seen
        [down(lo_x / F(FX0)), 0.0, 1.0],        # 5 one ulp outside
        [0.0, 0.0, -3.0],                       # 6 behind the camera
        [np.nan, 0.0, 2.0],                     # 7 a NaN position
        [0.0, np.inf, 2.0],                     # 8 an infinite one
        [0.1, 0.1, 2.0],                        # 9 seen, but the row is invalid
        [0.0, 0.0, 0.0],                        # 10 at the camera centre: 0 / 0
        [0.2, -0.1, 4.0],                       # 11 plainly seen
    ], dtype=F)
    assert len(edge) == EDGE_ROWS
    cloud = np.concatenate([rng.uniform(-4, 4, (n, 2)), rng.uniform(-3, 9, (n, 1))], axis=1).astype(F)
    cloud[::9] *= F(40.0)                                       # far outside every frame
    pc = np.concatenate([edge, cloud])[:n] if n > 1 else np.array([[0.2, -0.1, 4.0]], dtype=F)[:n]
    mask = (rng.uniform(size=n) < 0.1).astype(np.int8)
    if n > 1:
        mask[:EDGE_ROWS] = 0
        mask[9] = 1
    else:
        mask[:] = 0
    return pc, mask


@functools.lru_cache(maxsize=None)
def rate_case(n, n_views):
    pc, mask = rate_points(n)
    views = view_rows(n_views)
    want = ref.rate(pc, mask, views, W, H, NEAR, MARGIN)
    for a in (pc, mask, views, want):
        a.setflags(write=False)
    return pc, mask, views, want


def gpu_rate(pc, mask, views, **kw):
    return filter3d.sampling_rate(dev(pc).reshape(-1, 3), dev(mask), dev(views).reshape(-1, 16), W, H, NEAR, MARGIN, **kw).cpu().numpy()


@pytest.mark.parametrize("n_views", VIEWS)
@pytest.mark.parametrize("n", ROWS)
def test_rate_equals_the_reference_bit_for_bit(n, n_views):
    pc, mask, views, want = rate_case(n, n_views)
    got = gpu_rate(pc, mask, views)
    assert got.shape == (n,) and np.array_equal(bits(got), bits(want))
    again = gpu_rate(pc, mask, views, out=torch.full((n,), -1.0, device=DEV))              # a second run, into a buffer that held something
    assert np.array_equal(bits(again), bits(got))
    if n_views == 0:
        assert np.all(np.isinf(got))
    if n == 700 and n_views > 0:
        assert np.all(np.isinf(got[mask == 1])) and np.all(np.isfinite(got[mask == 0])) and np.all(got[mask == 0] > 0)
        smallest = got[mask == 0].min()
        assert (got[mask == 0] == smallest).sum() > 20, "rows no view sees take the smallest rate"
        assert len(np.unique(got[mask == 0])) > 100


def test_rate_at_the_edges_of_the_comparisons_under_one_view():
    pc, mask, views, want = rate_case(700, 1)
    got = gpu_rate(pc, mask, views)
    assert np.array_equal(bits(got), bits(want))
    smallest = got[mask == 0].min()
    fm = F(max(FX0, FY0))                                   # fx != fy: the larger one
    assert got[1] == fm / np.nextafter(F(NEAR), F(np.inf)) and got[2] == fm and got[4] == fm and got[11] == fm / F(4.0)
    for row in (0, 3, 5, 6, 7, 8, 10):                      # not seen: on the near plane, an ulp outside, behind, NaN, inf, 0 / 0
        assert got[row] == smallest, row
    assert np.isinf(got[9])
    assert FX0 != FY0 and got[11] != F(FX0) / F(4.0)


@pytest.mark.parametrize("n", ROWS)
def test_rate_when_no_view_sees_any_row(n):
    pc, mask = rate_points(n)
    pc = pc.copy()
    pc[:, 2] = -np.abs(pc[:, 2]) - 1.0                      # everything behind every camera (they all look along about +z)
    views = view_rows(17)
    want = ref.rate(pc, mask, views, W, H, NEAR, MARGIN)
    got = gpu_rate(pc, mask, views)
    assert np.array_equal(bits(got), bits(want)) and np.all(np.isinf(got)) and got.shape == (n,)


# ---- the transform ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def apply_case(n):
    """rows whose log-scales span -12 .. 3, logits -20 .. 40 and filter widths 1e-6 .. 10 independently (f >> s and f << s
    both occur), quaternions that are not unit, with identity rows: rate +inf, rate NaN"""
    rng = np.random.default_rng(17 + n)
    feat = rng.normal(0.0, 1.0, (n, 56)).astype(F)
    feat[:, :4] *= rng.uniform(0.2, 3.0, (n, 1)).astype(F)
    feat[:, 4:7] = rng.uniform(-12.0, 3.0, (n, 3))
    feat[:, 7] = rng.uniform(-20.0, 40.0, n)
    k = ref.filter_k(0.2, 2)
    f = np.exp(rng.uniform(np.log(1e-6), np.log(10.0), n))
    rate = (k / f).astype(F)
    if n > 1:
        feat[0, 4:7], rate[0] = [-12.0, -12.0, -12.0], F(k / 10.0)          # f >> s
        feat[1, 4:7], rate[1] = [3.0, 3.0, 3.0], F(k / 1e-6)                # f << s
        feat[2, 7], feat[3, 7] = 40.0, -20.0
        feat[4, :4] = ref.normalised_quaternions(ref.normalised_quaternions(ref.normalised_quaternions(feat[4:5, :4])))[0]
        rate[5::10] = np.inf
        rate[6::50] = np.nan
    grad = rng.normal(0.0, 1.0, (n, 56)).astype(F)
    grad[::7, 7] = 0.0
    grad[::5, 4:7] = 0.0
    grad[3::11, 5] = -0.0
    out, after = ref.apply(feat, rate, k)
    g64, mag = ref.apply_backward_f64(grad, feat, rate, k)
    c = dict(feat=feat, rate=rate, k=k, grad=grad, out=out, after=after, g64=g64, mag=mag, identity=~(ref.filter_width(rate, k) > 0))
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def test_the_apply_cases_cover_what_they_should():
    c = apply_case(700)
    f = ref.filter_width(c["rate"], c["k"])
    s = np.exp(c["feat"][:, 4:7].astype(np.float64))
    on = ~c["identity"]
    assert f[on].min() < 2e-6 and f[on].max() > 5.0 and (f[on, None] > 1e3 * s[on]).any() and (f[on, None] < 1e-3 * s[on]).any()
    assert c["feat"][:, 4:7].min() < -11.5 and c["feat"][:, 4:7].max() > 2.5
    assert c["feat"][:, 7].min() <= -19.0 and c["feat"][:, 7].max() >= 39.0
    assert 60 < c["identity"].sum() < 120 and np.isnan(c["rate"]).any() and np.isinf(c["rate"]).any()
    assert np.all(np.isfinite(c["out"][on])), "no logit may saturate"
    sig = 1.0 / (1.0 + np.exp(-c["feat"][:, 7].astype(np.float64)))
    assert (sig.astype(F)[on] == 1.0).sum() > 100, "sigmoid(a) must round to 1 in float32 in many rows"


@pytest.mark.parametrize("n", ROWS)
def test_apply_equals_the_reference(n):
    c = apply_case(n)
    feat = dev(c["feat"]).reshape(n, 56)
    got = filter3d.apply_forward(feat, dev(c["rate"]), c["k"]).cpu().numpy()
    after = feat.cpu().numpy()
    keep = [col for col in range(56) if col not in (4, 5, 6, 7)]
    assert got.shape == (n, 56)
    assert np.array_equal(bits(got[:, keep]), bits(c["out"][:, keep]))
    ident = c["identity"]
    assert np.array_equal(bits(got[ident]), bits(c["feat"][ident])) and np.array_equal(bits(after[ident]), bits(c["feat"][ident]))
    distance = ref.ulp_distance(got[:, 4:8], c["out"][:, 4:8])
    print(f"N={n}: {int((distance != 0).sum())} of {distance.size} float64-path elements differ from the reference, all by {int(distance.max()) if n else 0} ulp at most")
    assert n == 0 or distance.max() <= 1
    # the input rows: quaternions normalised as k_project does, nothing else moved; a normalised row keeps its bits
    assert np.array_equal(bits(after), bits(c["after"]))
    assert np.array_equal(bits(after[~ident, :4]), bits(ref.normalised_quaternions(c["feat"][~ident, :4])))
    if n > 1:
        assert np.array_equal(bits(after[4, :4]), bits(c["feat"][4, :4])) and not ident[4]
        moved = (bits(after[:, :4]) != bits(c["feat"][:, :4])).any(axis=1)
        assert moved[~ident].mean() > 0.9 and not moved[ident].any()
    # a zero filter: the identity on every row, input untouched
    feat0 = dev(c["feat"]).reshape(n, 56)
    same = filter3d.apply_forward(feat0, dev(c["rate"]), 0.0)
    assert torch.equal(same.view(torch.int32), feat0.view(torch.int32)) and np.array_equal(bits(feat0.cpu().numpy()), bits(c["feat"]))
    # two runs, the same bits
    again = filter3d.apply_forward(dev(c["feat"]).reshape(n, 56), dev(c["rate"]), c["k"]).cpu().numpy()
    assert np.array_equal(bits(again), bits(got))


@pytest.mark.parametrize("n", ROWS)
def test_apply_backward_is_within_one_ulp_of_float64(n):
    c = apply_case(n)
    feat, rate, grad = dev(c["feat"]).reshape(n, 56), dev(c["rate"]), dev(c["grad"]).reshape(n, 56)
    got_t = filter3d.apply_backward(grad, feat, rate, c["k"])
    got = got_t.cpu().numpy()
    assert np.array_equal(bits(feat.cpu().numpy()), bits(c["feat"])), "the backward reads the features only"
    keep = [col for col in range(56) if col not in (4, 5, 6, 7)]
    assert np.array_equal(bits(got[:, keep]), bits(c["grad"][:, keep]))
    ident = c["identity"]
    assert np.array_equal(bits(got[ident]), bits(c["grad"][ident]))
    want, mag = c["g64"][:, 4:8], c["mag"][:, 4:8]
    error, bound = np.abs(got[:, 4:8].astype(np.float64) - want), ref.ulp_of(want) + 1e-12 * mag
    if n:
        print(f"N={n}: largest error / bound {np.nanmax(error / bound):.3f}; {int((bits(got[:, 4:8]) != bits(want.astype(F))).sum())} "
              f"of {want.size} elements differ from the rounded float64 value")
    assert np.all(error <= bound)
    # zero upstream values: exact zeros in the rows that are computed
    on = ~ident
    zero_a, zero_ls = c["grad"][:, 7] == 0, (c["grad"][:, 4:7] == 0).all(axis=1)
    assert not got[on & zero_a, 7].any() and not np.signbit(got[on & zero_a, 7]).any()
    assert not got[on & zero_a & zero_ls, 4:7].any() and not np.signbit(got[on & zero_a & zero_ls, 4:7]).any()
    zeros = filter3d.apply_backward(torch.zeros_like(grad), feat, rate, c["k"])
    assert not bool(zeros.any()) and not bool(torch.signbit(zeros).any())
    # in place gives the same bits
    inplace = grad.clone()
    assert filter3d.apply_backward(inplace, feat, rate, c["k"], out=inplace) is inplace
    assert torch.equal(inplace.view(torch.int32), got_t.view(torch.int32))
    # autograd through filter3d.apply: the same two tensors, and the incoming gradient left alone
    x = dev(c["feat"]).reshape(n, 56).requires_grad_(True)
    y = filter3d.apply(x, rate, c["k"])
    upstream = grad.clone()
    y.backward(upstream)
    assert torch.equal(y.detach().view(torch.int32), filter3d.apply_forward(dev(c["feat"]).reshape(n, 56), rate, c["k"]).view(torch.int32))
    assert torch.equal(x.grad.view(torch.int32), got_t.view(torch.int32))
    assert torch.equal(upstream.view(torch.int32), grad.view(torch.int32))


# ---- through the rasteriser -------------------------------------------------------------------------------------------------
def scene_tensors(n):
    s = TU.ground_truth_scene()
    return SimpleNamespace(point_cloud=dev(s.point_cloud[:n]).reshape(n, 3), point_cloud_features=dev(s.point_cloud_features[:n]).reshape(n, 56),
                           point_invalid_mask=dev(s.point_invalid_mask[:n]), point_object_id=dev(s.point_object_id[:n]),
                           intrinsics=dev(s.camera_intrinsics))


def dataset_views(scene):
    from taichi_3d_gaussian_splatting_amd.utils import quaternion_to_rotation_matrix_torch
    poses = []
    for view in range(8):
        q, t = view_pose(view, 8)
        T = np.eye(4)
        T[:3, :3] = quaternion_to_rotation_matrix_torch(torch.tensor(q, dtype=torch.float64))[0].numpy()
        T[:3, 3] = t[0]
        poses.append(T)
    return filter3d.view_table(np.stack(poses), scene.intrinsics, device=DEV)


def render(module, scene, features, view=3):
    q, t = view_pose(view, 8)
    with torch.no_grad():
        return module(Rast.GaussianPointCloudRasterisationInput(
            point_cloud=scene.point_cloud, point_cloud_features=features, point_object_id=scene.point_object_id,
            point_invalid_mask=scene.point_invalid_mask, camera_info=CameraInfo(scene.intrinsics, TU.H, TU.W, 0),
            q_pointcloud_camera=dev(q), t_pointcloud_camera=dev(t), color_max_sh_band=3))[0]


@pytest.mark.parametrize("n", [TU.N_POINTS, 0])
def test_rendering_the_filtered_features_equals_rendering_the_fused_scene(n):
    module = Rast(Rast.GaussianPointCloudRasterisationConfig())
    a, b, plain = scene_tensors(n), scene_tensors(n), scene_tensors(n)
    original = a.point_cloud_features.clone()
    # a variance far above the default, so that the filter shows at this resolution
    config = Filter3DConfig(variance=4.0)
    fa, fb = Filter3D(config, a, dataset_views(a), width=TU.W, height=TU.H), Filter3D(config, b, dataset_views(b), width=TU.W, height=TU.H)
    assert torch.equal(fa.rate.view(torch.int32), fb.rate.view(torch.int32)) and fa.refreshes == 1
    filtered = fa.features(1)
    assert filtered.shape == (n, 56)
    image_a = render(module, a, filtered)
    assert fb.fuse_(b) is b
    image_b = render(module, b, b.point_cloud_features)
    assert torch.equal(image_a.view(torch.int32), image_b.view(torch.int32))
    assert torch.equal(a.point_cloud_features[:, 4:].view(torch.int32), original[:, 4:].view(torch.int32)), "features() leaves the scene raw"
    if n:
        assert bool(torch.isfinite(fa.rate).all()) and not torch.equal(image_a, render(module, plain, plain.point_cloud_features))
        assert bool((b.point_cloud_features[:, 4:7] > original[:, 4:7]).all()) and bool((b.point_cloud_features[:, 7] < original[:, 7]).all())


@pytest.mark.parametrize("n", [TU.N_POINTS, 0])
def test_a_table_of_infinite_rates_renders_as_no_filter(n):
    module = Rast(Rast.GaussianPointCloudRasterisationConfig())
    a, plain = scene_tensors(n), scene_tensors(n)
    filt = Filter3D(Filter3DConfig(), a)                    # no views, never refreshed: every rate +inf
    assert bool(torch.isinf(filt.rate).all())
    image = render(module, a, filt.features(4))
    want = render(module, plain, plain.point_cloud_features)
    assert torch.equal(image.view(torch.int32), want.view(torch.int32))
    # the rows the rasteriser normalised in the plain scene are the ones apply() normalises, to the same bits
    if n:
        seen = Filter3D(Filter3DConfig(), a, dataset_views(a), width=TU.W, height=TU.H)
        original = scene_tensors(n).point_cloud_features
        seen.features(1)
        rewritten = (plain.point_cloud_features[:, :4].view(torch.int32) != original[:, :4].view(torch.int32)).any(dim=1)
        assert int(rewritten.sum()) > 0
        assert torch.equal(a.point_cloud_features[rewritten, :4].view(torch.int32), plain.point_cloud_features[rewritten, :4].view(torch.int32))
    with pytest.raises(ValueError, match="no views"):
        filt.refresh()
