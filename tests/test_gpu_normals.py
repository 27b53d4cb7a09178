"""GPU (-m gpu): gs_gaussian_normals_* and gs_normal_consistency_* (include/gs_normals.h) through normals.py, against the
float64 restatement tests/normals_ref.py (pinned by test_normals_ref_host.py), and the term's autograd end to end.

Row counts: 1, 63, 64, 65 (a wave and its neighbours), 256, 257 (a block and one row of the next), 1025 (five blocks).  Picture
sizes: those of test_gpu_geometry.py -- 1x1 .. 2x2 (no normal at all), 3x3 (one), 5x4 (the smallest width the four-pixels-per-lane
path takes), partial tiles and halos on every side, a width that is a multiple of 4 and one that is not, and 528x600 = 330
tiles, more than the finishing block has threads.

Bars, from the design and not from the results: a value is a float64 result rounded once to f32, 2^-24 relative; the bar is
2^-22, four times that, relative to the summed magnitude of what was gathered into the element, plus the f32 denormal floor.
Counts are exact, and every element no selected term reaches is +0 with the sign bit clear.  Every element is compared."""
import functools

import numpy as np
import pytest
import torch

import normals_ref as R
from taichi_3d_gaussian_splatting_amd import geometry, normals

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TH, TW = geometry.TILE_H, geometry.TILE_W
EMPTY = [(1, 1), (1, 9), (9, 1), (2, 2)]
SMALL = [(3, 3), (5, 4), (TH + 1, TW + 1), (2 * TH + 3, 3 * TW + 2), (19, 132)]
LARGE = (528, 600)
ROWS = [1, 63, 64, 65, 256, 257, 1025]
BAR = 2.0 ** -22
FLOOR = 2.0 ** -149
K = (310.5, 305.25, 97.75, 40.5)
JUMP, MIN_LENGTH = 0.1, 0.5


def dev(v, misaligned=False):
    """the array on the device; misaligned: one float past a 16-byte boundary"""
    if v is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(v))
    if not misaligned:
        out = t.to(DEV).contiguous()
        assert out.data_ptr() % 16 == 0
        return out
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=DEV)
    out = buf[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def close(got, want, magnitude, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.isfinite(got).all(), what
    err, bar = np.abs(got - want), BAR * np.asarray(magnitude, dtype=np.float64) + FLOOR
    worst = float(np.max(err / bar)) if err.size else 0.0
    print(f"{what}: worst error / bar {worst:.3g} over {err.size} elements")
    assert np.all(err <= bar), (what, worst)


# ---- the per-row kernels ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gaussians(n, n_objects):
    """numpy rows: quaternions of length 0.5 .. 2, every axis the shortest somewhere; planted (where n allows): the tie
    log s_0 == log s_1 < log s_2, a NaN in q, an inf position, a zero quaternion, and a flipped beside an unflipped row"""
    rng = np.random.default_rng(100 * n + n_objects)
    pc = rng.uniform(-2.0, 2.0, (n, 3)).astype(np.float32)
    f = rng.normal(size=(n, 56)).astype(np.float32)
    q = rng.normal(size=(n, 4))
    f[:, :4] = q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (n, 1))
    f[:, 4:7] = rng.uniform(-4.0, -1.0, (n, 3))
    q_pc = rng.normal(size=(n_objects, 4))
    q_pc = (q_pc / np.linalg.norm(q_pc, axis=1, keepdims=True)).astype(np.float32)
    t_pc = (rng.uniform(-1.0, 1.0, (n_objects, 3)) + [0, 0, -6]).astype(np.float32)
    ids = rng.integers(0, n_objects, n).astype(np.int32) if n_objects > 1 else None
    g = rng.normal(size=(n, 3)).astype(np.float32)
    planted = {}
    if n >= 63:
        f[3, 4:7] = (-2.5, -2.5, -1.0)
        f[5, 2] = np.nan
        pc[7, 1] = np.inf
        f[9, :4] = 0.0
        f[11, 6] = -np.inf
        # rows 20 and 21: the same Gaussian and the same upstream at camera-frame positions (0, 0, 2) and (0, 0, -2) of object 0:
        # exactly one of them is flipped
        f[20], g[20] = f[21], g[21]
        if ids is not None:
            ids[20] = ids[21] = 0
        Pm = R.rotation(q_pc[:1].astype(np.float64))[0]
        pc[20] = (t_pc[0] + 2.0 * Pm[:, 2]).astype(np.float32)
        pc[21] = (t_pc[0] - 2.0 * Pm[:, 2]).astype(np.float32)
        planted = dict(tie=3, zeroed=(5, 7, 9, 11), pair=(20, 21))
    return pc, f, q_pc, t_pc, ids, g, planted


def run_rows(pc, f, q_pc, t_pc, ids, g):
    d = [dev(v) for v in (pc, f, q_pc, t_pc, ids, g)]
    result = []
    for _ in range(2):                      # two runs: the same bits
        n_out = normals.gaussian_normals_forward(d[0], d[1], d[2], d[3], d[4], out=torch.full((len(pc), 3), np.nan, device=DEV))
        g_out = normals.gaussian_normals_backward(d[0], d[1], d[2], d[3], d[4], d[5], out=torch.full((len(pc), 56), np.nan, device=DEV))
        result.append((n_out.cpu(), g_out.cpu()))
    assert torch.equal(bits(result[0][0]), bits(result[1][0])) and torch.equal(bits(result[0][1]), bits(result[1][1]))
    return result[0]


@pytest.mark.parametrize("n_objects", [1, 2])
@pytest.mark.parametrize("n", ROWS)
def test_gaussian_normals_match_the_float64_restatement(n, n_objects):
    pc, f, q_pc, t_pc, ids, g, planted = gaussians(n, n_objects)
    assert (ids is None) == (n_objects == 1)
    got_n, got_g = run_rows(pc, f, q_pc, t_pc, ids, g)
    want_n, mag_n = R.gaussian_normals_forward(pc, f, q_pc, t_pc, ids)
    want_g, mag_g = R.gaussian_normals_backward(pc, f, q_pc, t_pc, ids, g)
    what = f"gaussian normals n {n} objects {n_objects}"
    close(got_n.numpy(), want_n, mag_n, what)
    close(got_g.numpy(), want_g, mag_g, what + " grad")
    assert not bits(got_g[:, 4:]).any(), "grad_features[:, 4:] is not all +0"
    rows = R._rows(pc, f, q_pc, t_pc, ids)
    assert not bits(got_n)[torch.from_numpy(~rows["ok"])].any() and not bits(got_g)[torch.from_numpy(~rows["ok"])].any()
    ok = rows["ok"]
    assert np.allclose(np.linalg.norm(got_n.numpy()[ok], axis=1), 1.0, atol=1e-5)
    assert np.all(np.einsum("nj,nj->n", got_n.numpy()[ok].astype(np.float64), rows["p"][ok]) <= 0)          # facing the camera
    if planted:
        assert rows["k"][planted["tie"]] == 0 and ok[planted["tie"]]
        c0 = R.rotation(f[planted["tie"], :4].astype(np.float64)[None])[0][:, 0]
        m0 = R.rotation(q_pc.astype(np.float64))[0 if ids is None else ids[planted["tie"]]].T @ (c0 / np.linalg.norm(c0))
        assert np.allclose(np.abs(got_n[planted["tie"]].numpy()), np.abs(m0), atol=1e-6)                    # column 0, not column 1
        for i in planted["zeroed"]:
            assert not ok[i] and not bits(got_n[i]).any() and not bits(got_g[i]).any()
        a, b = planted["pair"]
        assert rows["flip"][a] != rows["flip"][b] and ok[a] and ok[b]
        assert np.array_equal(got_n[a].numpy(), -got_n[b].numpy()) and got_n[a].abs().max() > 0.5          # each faces its camera side
        assert np.array_equal(got_g[a, :4].numpy(), -got_g[b, :4].numpy()) and got_g[a, :4].abs().max() > 0
        assert set(rows["k"][ok]) == {0, 1, 2}
    else:
        assert ok.all()


def test_gaussian_normals_autograd_reaches_the_quaternion_only():
    pc, f, q_pc, t_pc, ids, g, _ = gaussians(257, 2)
    d_pc, d_f, d_q, d_t, d_ids, d_g = (dev(v) for v in (pc, f, q_pc, t_pc, ids, g))
    d_f.requires_grad_(True)
    d_pc.requires_grad_(True)
    out = normals.gaussian_normals(d_pc, d_f, d_q, d_t, d_ids)
    (out * d_g).sum().backward()
    assert d_pc.grad is None
    want = normals.gaussian_normals_backward(d_pc.detach(), d_f.detach(), d_q, d_t, d_ids, d_g)
    assert torch.equal(bits(d_f.grad), bits(want)) and d_f.grad[:, :4].abs().max() > 0


# ---- the consistency kernels ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(h, w):
    """numpy float32: a wavy depth with a planted step edge, a constant block and holes; rendered normals near the surface's,
    0.6 .. 1 long, with some below min_length; weights with zero, negative and NaN entries"""
    rng = np.random.default_rng(1000 * h + w)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    D = 2.0 + 0.02 * np.sin(xx / 7.0) + 0.03 * np.cos(yy / 5.0) + 0.002 * rng.uniform(-1, 1, (h, w))
    D[:, w // 2:] += 1.5                                              # a step edge: max_rel_jump cuts the normals across it
    D[rng.uniform(size=(h, w)) < 0.03] = 0.0
    if h >= 11 and w >= 11:
        D[4:9, 4:9] = 2.03125                                         # constant depth
    Rn = np.stack([0.3 * rng.normal(size=(h, w)), 0.3 * rng.normal(size=(h, w)), -np.ones((h, w))], axis=2)
    Rn = Rn / np.linalg.norm(Rn, axis=2, keepdims=True) * rng.uniform(0.6, 1.0, (h, w, 1))
    Rn[rng.uniform(size=(h, w)) < 0.08] *= 0.5                        # 0.3 .. 0.5: below min_length
    w_p = rng.uniform(0.1, 1.0, (h, w))
    off = rng.uniform(size=(h, w))
    w_p[off < 0.12] = np.nan
    w_p[off < 0.08] = -1.0
    w_p[off < 0.04] = 0.0
    if h >= 3 and w >= 3:
        D[0:3, 0:3] = np.array([[2.0, 2.04, 2.0], [2.03, 2.02, 2.05], [2.0, 2.06, 2.0]])      # the first normal exists
        w_p[1, 1], Rn[1, 1] = 0.5, (0.1, -0.2, -0.8)
    return tuple(np.ascontiguousarray(v, dtype=np.float32) for v in (D, Rn, w_p))


def run_consistency(D, Rn, w_p, jump=JUMP, min_length=MIN_LENGTH, upstream=None, misaligned=False):
    d = [dev(v, misaligned) for v in (D, Rn, w_p)]
    up = None if upstream is None else torch.tensor([upstream], dtype=torch.float32, device=DEV)
    result = []
    for _ in range(2):                      # two runs: the same bits
        terms = normals.normal_consistency_forward(d[0], d[1], K, d[2], jump, min_length)
        gd, gr = normals.normal_consistency_backward(d[0], d[1], K, d[2], jump, min_length, terms, up,
                                                     out_depth=dev(np.full(D.shape, np.nan, np.float32), misaligned),
                                                     out_rendered=dev(np.full(Rn.shape, np.nan, np.float32), misaligned))
        result.append((terms.cpu(), gd.cpu(), gr.cpu()))
    for a, b in zip(*result):
        assert torch.equal(bits(a), bits(b))
    return result[0]


def compare_consistency(h, w, jump=JUMP, with_wp=True, upstream=None, min_length=MIN_LENGTH):
    D, Rn, w_p = scene(h, w)
    w_p = w_p if with_wp else None
    what = f"consistency {h}x{w} jump {jump} w_p {with_wp} min_length {min_length}"
    terms, gd, gr = run_consistency(D, Rn, w_p, jump, min_length, upstream)
    _, values, selected = R.normal_consistency_forward(D, K, Rn, w_p, jump, min_length)
    assert torch.isfinite(terms).all() and not terms[4:].any()
    assert terms[2].item() == values["count"], what
    close(terms[0].item(), values["L"], abs(values["L"]), what + " L")
    close(terms[1].item(), values["S_w"], values["S_w"], what + " S_w")
    close(terms[3].item(), values["mean_cos"], abs(values["mean_cos"]), what + " mean cos")
    want_d, mag_d, touched, want_r, mag_r, sel = R.normal_consistency_backward(D, K, Rn, w_p, jump, min_length, terms.numpy(),
                                                                               1.0 if upstream is None else upstream)
    close(gd.numpy(), want_d, mag_d, what + " grad_D")
    close(gr.numpy(), want_r, mag_r, what + " grad_R")
    assert not bits(gd)[torch.from_numpy(~touched)].any(), what + ": an element of grad_D no term reaches is not +0"
    assert not bits(gr)[torch.from_numpy(~sel)].any(), what + ": an element of grad_R at an unselected pixel is not +0"
    return values["count"]


@pytest.mark.parametrize("h,w", EMPTY)
def test_an_image_too_small_for_a_normal_gives_zeros(h, w):
    assert compare_consistency(h, w) == 0
    terms, gd, gr = run_consistency(*scene(h, w))
    assert not bits(terms).any() and not bits(gd).any() and not bits(gr).any()


@pytest.mark.parametrize("h,w", SMALL)
def test_consistency_matches_the_float64_restatement(h, w):
    assert compare_consistency(h, w) >= 1
    assert compare_consistency(h, w, jump=0.0, with_wp=False) >= 1
    assert compare_consistency(h, w, upstream=-0.75) >= 1
    assert compare_consistency(h, w, min_length=0.75) >= 1
    if (h, w) == SMALL[3]:
        D, Rn, w_p = scene(h, w)
        assert w % 4 != 0
        free = R.normal_consistency_forward(D, K, Rn, w_p, 0.0, MIN_LENGTH)[2]
        cut = R.normal_consistency_forward(D, K, Rn, w_p, JUMP, MIN_LENGTH)[2]
        edge = np.zeros((h, w), dtype=bool)
        edge[:, w // 2 - 1:w // 2 + 1] = True
        assert (free & edge).sum() > 10 and not (cut & edge).any()                        # the step edge is cut by max_rel_jump
        short = np.linalg.norm(Rn.astype(np.float64), axis=2) < MIN_LENGTH
        assert short.sum() > 50 and not (cut & short).any()
        assert np.all(D[4:9, 4:9] == D[4, 4]) and D[4, 4] > 0                              # the constant-depth block is in the picture


def test_more_tiles_than_the_finishing_block_has_threads():
    h, w = LARGE
    assert -(-h // TH) * -(-w // TW) > geometry.FINISH_THREADS
    assert compare_consistency(h, w, upstream=3.0) > 100000


def test_what_is_not_selected_changes_no_bit():
    """NaN, inf and negative values in D at holes, in R where the weight is off, where R was too short, and where no depth
    normal exists; in the weights where they were off: every sum and every gradient keeps its bits"""
    h, w = SMALL[3]
    D, Rn, w_p = (v.copy() for v in scene(h, w))
    clean = run_consistency(D, Rn, w_p)
    poison = np.array([np.nan, np.inf, -np.inf, -1.0], dtype=np.float32)
    with np.errstate(invalid="ignore"):
        holes, off = D == 0, ~(w_p > 0)
    exists = R.G.normal_fields(D, K, JUMP)["exists"]
    short = np.linalg.norm(Rn.astype(np.float64), axis=2) < MIN_LENGTH
    assert holes.sum() > 20 and off.sum() > 20 and short.sum() > 20 and (~exists).sum() > 20
    D[holes] = np.resize(poison, holes.sum())
    Rn[off | ~exists] = np.resize(poison[:3], ((off | ~exists).sum(), 3))
    Rn[short & ~off & exists, 1] = np.nan                   # an unusable blend stays unusable
    w_p[off] = np.resize(poison[[0, 2, 3]], off.sum())
    again = run_consistency(D, Rn, w_p)
    for a, b in zip(clean, again):
        assert torch.equal(bits(a), bits(b))
    assert clean[0][2].item() > 100


@pytest.mark.parametrize("h,w", [SMALL[1], SMALL[4], LARGE])
def test_misaligned_planes_give_the_bits_of_aligned_ones(h, w):
    assert w % 4 == 0
    a, b = run_consistency(*scene(h, w)), run_consistency(*scene(h, w), misaligned=True)
    for x, y in zip(a, b):
        assert torch.equal(bits(x), bits(y))


def test_nothing_selected_gives_eight_zeros_and_zero_gradients():
    h, w = SMALL[2]
    D, Rn, w_p = scene(h, w)
    for out in (run_consistency(D, Rn, np.zeros_like(w_p)), run_consistency(D, Rn * 0.4, None), run_consistency(np.zeros_like(D), Rn, w_p),
                run_consistency(D, Rn, w_p, min_length=1.5)):
        assert all(not bits(v).any() for v in out)


def test_autograd_scales_both_gradients_by_the_upstream():
    """(2.5 * loss).backward() against 2.5 times the unit-upstream gradients: both are float64 results rounded once, so they
    differ by at most the two roundings, 2^-23 of the value"""
    h, w = SMALL[3]
    D, Rn, w_p = (dev(v) for v in scene(h, w))
    leaves = [(D.clone().requires_grad_(True), Rn.clone().requires_grad_(True)) for _ in range(2)]
    loss = normals.normal_consistency(*leaves[0], K, w_p, JUMP, MIN_LENGTH)
    assert loss.terms.shape == (8,) and loss.item() == loss.terms[0].item() and loss.item() > 0
    loss.backward()
    (2.5 * normals.normal_consistency(*leaves[1], K, w_p, JUMP, MIN_LENGTH)).backward()
    for one, other in zip(*leaves):
        unit, scaled = one.grad.double().cpu().numpy(), other.grad.double().cpu().numpy()
        assert np.abs(unit).max() > 0
        assert np.all(np.abs(scaled - 2.5 * unit) <= 2.0 ** -23 * np.abs(2.5 * unit) + FLOOR)
        assert not bits(other.grad)[bits(one.grad) == 0].any()
    # a node asked for one gradient only gives that one
    d = D.clone().requires_grad_(True)
    normals.normal_consistency(d, Rn, K, w_p, JUMP, MIN_LENGTH).backward()
    assert torch.equal(bits(d.grad), bits(leaves[0][0].grad))


def test_work_memory_belongs_to_the_context_and_a_call_allocates_nothing():
    from taichi_3d_gaussian_splatting_amd import _native
    h, w = LARGE
    D, Rn, w_p = (dev(v) for v in scene(h, w))
    normals.normal_consistency_forward(D, Rn, K, w_p, JUMP, MIN_LENGTH)
    L, ctx = _native.lib(), _native.shared_ctx(D.device)
    before = L.gs_ctx_device_bytes(ctx)
    assert before >= -(-h // TH) * -(-w // TW) * 4 * 8
    free = torch.cuda.mem_get_info()[0]
    gd, gr = torch.empty_like(D), torch.empty_like(Rn)
    for _ in range(3):
        terms = normals.normal_consistency_forward(D, Rn, K, w_p, JUMP, MIN_LENGTH)
        normals.normal_consistency_backward(D, Rn, K, w_p, JUMP, MIN_LENGTH, terms, out_depth=gd, out_rendered=gr)
    torch.cuda.synchronize()
    assert L.gs_ctx_device_bytes(ctx) == before
    assert torch.cuda.mem_get_info()[0] >= free - (64 << 20)


# ---- autograd end to end ----------------------------------------------------------------------------------------------------------
def test_the_term_reaches_points_and_quaternions_through_depth_and_channels():
    """48x64, a few hundred Gaussians: rast(...) with differentiable_depth, rendered_normals, normal_consistency(...).backward().
    The gradient of feature columns 0..3 is the rasteriser's own q gradient (of the depth gradient alone) plus
    gs_gaussian_normals_backward of gs_channels_backward of grad_R, composed here from the library calls and added in f32 (a sum
    of two: its order does not matter)."""
    from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast, channels
    from taichi_3d_gaussian_splatting_amd.synthetic import scene_input, synth, view_pose
    H, W = 48, 64
    s = synth(300, W, H, 0.08, sh_deg=3, seed=2)
    q, t = view_pose(0, 1)
    config = Rast.GaussianPointCloudRasterisationConfig()
    config.differentiable_depth = True
    rast = Rast(config)
    inp = scene_input(s, q, t, DEV, band=3, requires_grad=True)
    image, depth, _ = rast(inp)
    frame = rast.last_frame
    Rn = normals.rendered_normals(rast, (inp.point_cloud, inp.point_cloud_features, inp.point_object_id),
                                  (inp.q_pointcloud_camera, inp.t_pointcloud_camera))
    assert tuple(Rn.shape) == (H, W, 3)
    loss = normals.normal_consistency(depth, Rn, inp.camera_info.camera_intrinsics, None, JUMP, 0.3)
    assert loss.terms[2].item() > 50 and 0 < loss.item() < 2
    loss.backward()
    g_pc, g_f = inp.point_cloud.grad, inp.point_cloud_features.grad
    assert g_pc is not None and g_pc.abs().max() > 0 and torch.isfinite(g_pc).all() and torch.isfinite(g_f).all()
    for column in range(8):
        assert g_f[:, column].abs().max() > 0, f"no gradient reaches feature column {column}"

    # by hand: the two library gradients of the loss, then each path's own backward
    K4 = geometry.intrinsics_tuple(inp.camera_info.camera_intrinsics)
    D_, R_ = depth.detach(), Rn.detach()
    gd, gr = normals.normal_consistency_backward(D_, R_, K4, None, JUMP, 0.3, loss.terms,
                                                 torch.ones(1, dtype=torch.float32, device=DEV))
    pc_, f_ = inp.point_cloud.detach(), inp.point_cloud_features.detach()
    grad_values = torch.empty(pc_.shape[0], 3, dtype=torch.float32, device=DEV)
    channels._bind()
    from taichi_3d_gaussian_splatting_amd import _native
    _native.call("gs_channels_backward", gr.device, frame._context.handle, channels._ticket(frame), gr.data_ptr(), 3, frame.last.data_ptr(),
                 grad_values.data_ptr())
    via_normals = normals.gaussian_normals_backward(pc_, f_, inp.q_pointcloud_camera, inp.t_pointcloud_camera, inp.point_object_id, grad_values)
    inp2 = scene_input(s, q, t, DEV, band=3, requires_grad=True)
    _, depth2, _ = rast(inp2)
    assert torch.equal(bits(depth2), bits(depth))
    depth2.backward(gd)
    via_depth = inp2.point_cloud_features.grad
    assert torch.equal(bits(inp2.point_cloud.grad), bits(g_pc))                        # positions: through the depth alone
    want = via_depth + via_normals
    assert torch.equal(bits(want[:, :4]), bits(g_f[:, :4])) and via_normals[:, :4].abs().max() > 0 and via_depth[:, :4].abs().max() > 0
    assert torch.equal(bits(want[:, 4:]), bits(g_f[:, 4:]))
