"""GPU (-m gpu): gs_depth_normals, gs_normal_loss_* and gs_depth_smooth_* (include/gs_geometry.h) through geometry.py, against the
float64 restatement tests/geometry_ref.py (pinned by test_geometry_ref_host.py).

Sizes (H, W): 1x1, 1x9, 9x1, 2x2 (no normal and no second-order term at all), 3x3 (one normal), 5x4 (the smallest width the
four-pixels-per-lane path takes), (TILE_H + 1) x (TILE_W + 1) and (2 TILE_H + 3) x (3 TILE_W + 2) (halos and partial tiles on
every side, pixel by pixel), 19x132 (the same with a width that is a multiple of 4) and 528x600 = 330 tiles: more than the 256
threads of the finishing block, so both of its loops run.

Bars, from the design and not from the results: a value is a float64 result rounded once to f32, 2^-24 relative; the bar is
2^-22, four times that, relative to the summed magnitude of the terms gathered into the element (for a forward term: to the
term), plus the f32 denormal floor.  What device and numpy differ by in float64 (exp, the order of the picture-wide sums, S_w
read back as f32 by the backward: one more f32 rounding, inside the 4x) is ten orders of magnitude below the rest.  Counts are
exact, and every element no selected term reaches is +0 with the sign bit clear.  Every element is compared, none left out:
where a residual is exactly 0 (the planted constant-depth block) both sides have |r|' = 0."""
import functools

import numpy as np
import pytest
import torch

import geometry_ref as R
from taichi_3d_gaussian_splatting_amd import geometry

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TH, TW = geometry.TILE_H, geometry.TILE_W
EMPTY = [(1, 1), (1, 9), (9, 1), (2, 2)]
SMALL = [(3, 3), (5, 4), (TH + 1, TW + 1), (2 * TH + 3, 3 * TW + 2), (19, 132)]
LARGE = (528, 600)
BAR = 2.0 ** -22
FLOOR = 2.0 ** -149
K = (310.5, 305.25, 97.75, 40.5)
JUMP = 0.1


@functools.lru_cache(maxsize=None)
def scene(h, w):
    """numpy float32 planes: a wavy depth with a planted step edge, a constant block and holes; a prior near the surface's
    normals with unusable pixels; weights with zeros; a guide"""
    rng = np.random.default_rng(1000 * h + w)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    D = 2.0 + 0.02 * np.sin(xx / 7.0) + 0.03 * np.cos(yy / 5.0) + 0.002 * rng.uniform(-1, 1, (h, w))
    D[:, w // 2:] += 1.5                                              # a step edge: max_rel_jump cuts the normals across it
    D[rng.uniform(size=(h, w)) < 0.03] = 0.0
    if h >= 11 and w >= 11:
        D[4:9, 4:9] = 2.03125                                         # constant: every residual in it is exactly 0
    N = np.stack([0.3 * rng.normal(size=(h, w)), 0.3 * rng.normal(size=(h, w)), -np.ones((h, w))])
    N = N / np.linalg.norm(N, axis=0)
    N[:, rng.uniform(size=(h, w)) < 0.05] *= 0.3                      # too short to be usable
    w_n = rng.uniform(0.1, 1.0, (h, w))
    w_n[rng.uniform(size=(h, w)) < 0.1] = 0.0
    w_p = rng.uniform(0.1, 1.0, (h, w))
    w_p[rng.uniform(size=(h, w)) < 0.1] = 0.0
    if h >= 3 and w >= 3:
        D[0:3, 0:3] = np.array([[2.0, 2.04, 2.0], [2.03, 2.02, 2.05], [2.0, 2.06, 2.0]])      # the first normal exists
        w_n[1, 1], w_p[1, 1], N[:, 1, 1] = 0.75, 0.5, (0.0, 0.0, -1.0)
    I = 0.5 + 0.5 * np.sin(xx / 3.0 + rng.uniform(0, 6, (3, 1, 1))) * np.cos(yy / 4.0) + 0.05 * rng.uniform(-1, 1, (3, h, w))
    return tuple(np.ascontiguousarray(v, dtype=np.float32) for v in (D, N, w_n, w_p, I))


def dev(v, misaligned=False):
    """the array on the device; misaligned: one float past a 16-byte boundary"""
    if v is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(v))
    if not misaligned:
        out = t.to(DEV).contiguous()
        assert out.data_ptr() % 16 == 0
        return out
    buf = torch.empty(t.numel() + 8, dtype=torch.float32, device=DEV)
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


def run_normals(D, jump, misaligned=False):
    out = geometry.depth_normals(dev(D, misaligned), K, jump, out=dev(np.zeros((3,) + D.shape, np.float32), misaligned))
    again = geometry.depth_normals(dev(D, misaligned), K, jump)
    assert torch.equal(bits(out), bits(again))
    return out.cpu()


def run_normal_loss(D, N, w_n, w_p, jump, flags, upstream=None, misaligned=False):
    d = [dev(v, misaligned) for v in (D, N, w_n, w_p)]
    up = None if upstream is None else torch.tensor([upstream], dtype=torch.float32, device=DEV)
    result = []
    for _ in range(2):                      # two runs: the same bits
        terms = geometry.normal_loss_forward(d[0], K, d[1], d[2], d[3], jump, flags)
        grad = geometry.normal_loss_backward(d[0], K, d[1], d[2], d[3], jump, flags, terms, up, out=dev(np.full(D.shape, np.nan, np.float32), misaligned))
        result.append((terms.cpu(), grad.cpu()))
    assert torch.equal(bits(result[0][0]), bits(result[1][0])) and torch.equal(bits(result[0][1]), bits(result[1][1]))
    return result[0]


def run_smooth(D, I, w_p, lam, flags, upstream=None, misaligned=False):
    d = [dev(v, misaligned) for v in (D, I, w_p)]
    up = None if upstream is None else torch.tensor([upstream], dtype=torch.float32, device=DEV)
    result = []
    for _ in range(2):
        terms = geometry.depth_smooth_forward(d[0], d[1], d[2], lam, flags)
        grad = geometry.depth_smooth_backward(d[0], d[1], d[2], lam, flags, terms, up, out=dev(np.full(D.shape, np.nan, np.float32), misaligned))
        result.append((terms.cpu(), grad.cpu()))
    assert torch.equal(bits(result[0][0]), bits(result[1][0])) and torch.equal(bits(result[0][1]), bits(result[1][1]))
    return result[0]


def check_terms(terms, values, what, mean_cos=False):
    assert torch.isfinite(terms).all() and not terms[4:].any()
    assert terms[2].item() == values["count"], what
    close(terms[0].item(), values["L"], abs(values["L"]), what + " L")
    close(terms[1].item(), values["S_w"], values["S_w"], what + " S_w")
    if mean_cos:
        close(terms[3].item(), values["mean_cos"], abs(values["mean_cos"]), what + " mean cos")
    else:
        assert terms[3].item() == 0.0


def check_grad(grad, want, magnitude, touched, what):
    close(grad.numpy(), want, magnitude, what)
    assert not bits(grad)[torch.from_numpy(~touched)].any(), what + ": an element no term reaches is not +0"


def compare_normals(h, w, jump):
    D = scene(h, w)[0]
    want, magnitude = R.depth_normals(D, K, jump)
    got = run_normals(D, jump)
    close(got.numpy(), want, magnitude, f"normals {h}x{w} jump {jump}")
    assert not bits(got)[torch.from_numpy(magnitude == 0)].any()
    return int((magnitude.sum(0) > 0).sum())


def compare_normal_loss(h, w, flags, jump=JUMP, with_wp=True, upstream=None):
    D, N, w_n, w_p, _ = scene(h, w)
    if flags & R.PRIOR_UNIT_RANGE:
        N = ((N.astype(np.float64) + 1.0) / 2.0).astype(np.float32)
    w_p = w_p if with_wp else None
    what = f"normal loss {h}x{w} flags {flags} jump {jump} w_p {with_wp}"
    terms, grad = run_normal_loss(D, N, w_n, w_p, jump, flags, upstream)
    _, values, _ = R.normal_loss_forward(D, K, N, w_n, w_p, jump, flags)
    check_terms(terms, values, what, mean_cos=True)
    want, magnitude, touched = R.normal_loss_backward(D, K, N, w_n, w_p, jump, flags, terms.numpy(), 1.0 if upstream is None else upstream)
    check_grad(grad, want, magnitude, touched, what + " grad")
    return values["count"]


def compare_smooth(h, w, flags, guided=True, with_wp=True, upstream=None, lam=10.0):
    D, _, _, w_p, I = scene(h, w)
    I, w_p = (I if guided else None), (w_p if with_wp else None)
    what = f"smoothness {h}x{w} flags {flags} guide {guided} w_p {with_wp}"
    terms, grad = run_smooth(D, I, w_p, lam, flags, upstream)
    _, values = R.depth_smooth_forward(D, I, w_p, lam, flags)
    check_terms(terms, values, what)
    want, magnitude, touched = R.depth_smooth_backward(D, I, w_p, lam, flags, terms.numpy(), 1.0 if upstream is None else upstream)
    check_grad(grad, want, magnitude, touched, what + " grad")
    return values["count"]


@pytest.mark.parametrize("h,w", EMPTY)
def test_an_image_too_small_for_a_term_gives_zeros(h, w):
    assert compare_normals(h, w, 0.0) == 0
    for flags in (0, R.PRIOR_FLIP_YZ):
        assert compare_normal_loss(h, w, flags) == 0
    counts = [compare_smooth(h, w, flags) for flags in (0, R.INVERSE, R.SECOND_ORDER)]      # a row of nine pixels has pairs and triples
    assert (h, w) != (1, 1) or counts == [0, 0, 0]
    assert (h, w) != (2, 2) or counts[2] == 0
    D, N, w_n, w_p, I = scene(h, w)
    terms, grad = run_normal_loss(D, N, w_n, w_p, JUMP, 0)
    assert not bits(terms).any() and not bits(grad).any()
    if (h, w) in ((1, 1), (2, 2)):
        terms, grad = run_smooth(D, I, w_p, 10.0, R.SECOND_ORDER)
        assert not bits(terms).any() and not bits(grad).any()


@pytest.mark.parametrize("h,w", SMALL)
def test_normals_and_losses_match_the_float64_restatement(h, w):
    assert compare_normals(h, w, 0.0) >= 1
    assert compare_normals(h, w, JUMP) >= 1
    for flags in (0, R.PRIOR_UNIT_RANGE, R.PRIOR_FLIP_YZ, R.NORMAL_FLAGS_ALL):        # each flag on its own, and both
        assert compare_normal_loss(h, w, flags) >= 1
    for flags in (0, R.INVERSE, R.SECOND_ORDER, R.SMOOTH_FLAGS_ALL):
        assert compare_smooth(h, w, flags) >= 1
    compare_normal_loss(h, w, 0, jump=0.0, with_wp=False)
    compare_smooth(h, w, R.INVERSE, guided=False, with_wp=False)
    compare_smooth(h, w, R.SECOND_ORDER, guided=False)
    compare_smooth(h, w, 0, lam=0.0)


def test_more_tiles_than_the_finishing_block_has_threads():
    h, w = LARGE
    tiles = -(-h // TH) * -(-w // TW)
    assert tiles > geometry.FINISH_THREADS and 0.25e6 < h * w < 0.4e6
    compare_normals(h, w, JUMP)
    assert compare_normal_loss(h, w, R.PRIOR_FLIP_YZ, upstream=-0.75) > 100000
    assert compare_smooth(h, w, R.INVERSE) > 300000
    assert compare_smooth(h, w, R.SECOND_ORDER, upstream=3.0) > 300000


def test_max_rel_jump_cuts_the_normals_across_a_step_edge():
    h, w = SMALL[3]
    D, N, w_n, w_p, _ = scene(h, w)
    free, cut = R.depth_normals(D, K, 0.0)[1].sum(0) > 0, R.depth_normals(D, K, JUMP)[1].sum(0) > 0
    edge = np.zeros((h, w), dtype=bool)
    edge[:, w // 2 - 1:w // 2 + 1] = True
    assert (free & edge).sum() > 10 and not (cut & edge).any() and np.array_equal(cut & ~edge, free & ~edge)
    got_free, got_cut = run_normals(D, 0.0).numpy(), run_normals(D, JUMP).numpy()
    assert np.array_equal(np.abs(got_free).sum(0) > 0, free) and np.array_equal(np.abs(got_cut).sum(0) > 0, cut)
    a = run_normal_loss(D, N, w_n, w_p, 0.0, 0)[0]
    b = run_normal_loss(D, N, w_n, w_p, JUMP, 0)[0]
    assert a[2].item() > b[2].item() > 0


def test_a_constant_depth_region_has_a_zero_subgradient():
    h, w = SMALL[2]
    D = scene(h, w)[0]
    assert np.all(D[4:9, 4:9] == D[4, 4]) and D[4, 4] > 0
    for flags in (0, R.INVERSE, R.SECOND_ORDER):
        _, grad = run_smooth(D, None, None, 10.0, flags)
        assert not grad[6, 6].any()                          # every term the centre takes part in has r == 0
        want, magnitude, touched = R.depth_smooth_backward(D, None, None, 10.0, flags, run_smooth(D, None, None, 10.0, flags)[0].numpy())
        assert touched[6, 6] and magnitude[6, 6] == 0 and want[6, 6] == 0


def test_what_is_not_selected_changes_no_bit():
    """NaN, inf and negative values in D at holes, in the prior and the guide under a zero weight, and in the weights where
    they were zero: every sum and every gradient keeps its bits"""
    h, w = SMALL[3]
    D, N, w_n, w_p, I = (v.copy() for v in scene(h, w))
    clean_n = [run_normal_loss(D, N, w_n, w_p, JUMP, f) for f in (0, R.PRIOR_FLIP_YZ)]
    clean_s = [run_smooth(D, I, w_p, 10.0, f) for f in (0, R.SMOOTH_FLAGS_ALL)]
    clean_d = run_normals(D, JUMP)
    poison = np.array([np.nan, np.inf, -np.inf, -1.0], dtype=np.float32)
    holes, off_n, off_p = D == 0, w_n == 0, w_p == 0
    assert holes.sum() > 20 and off_n.sum() > 20 and off_p.sum() > 20
    D[holes] = np.resize(poison, holes.sum())
    N[:, off_n | off_p] = np.resize(poison[:3], (3, (off_n | off_p).sum()))
    I[:, off_p] = np.resize(poison[:3], (3, off_p.sum()))
    w_n[off_n] = np.resize(poison[[0, 2, 3]], off_n.sum())
    w_p[off_p] = np.resize(poison[[0, 2, 3]], off_p.sum())
    for clean, f in zip(clean_n, (0, R.PRIOR_FLIP_YZ)):
        terms, grad = run_normal_loss(D, N, w_n, w_p, JUMP, f)
        assert torch.equal(bits(terms), bits(clean[0])) and torch.equal(bits(grad), bits(clean[1]))
    for clean, f in zip(clean_s, (0, R.SMOOTH_FLAGS_ALL)):
        terms, grad = run_smooth(D, I, w_p, 10.0, f)
        assert torch.equal(bits(terms), bits(clean[0])) and torch.equal(bits(grad), bits(clean[1]))
    assert torch.equal(bits(run_normals(D, JUMP)), bits(clean_d))
    # a non-finite guide difference unselects its pairs even under a weight: the restatement agrees
    I2 = scene(h, w)[4].copy()
    I2[1, 5, 7] = np.inf
    terms, grad = run_smooth(scene(h, w)[0], I2, None, 10.0, 0)
    _, values = R.depth_smooth_forward(scene(h, w)[0], I2, None, 10.0, 0)
    check_terms(terms, values, "guide with an inf")


@pytest.mark.parametrize("h,w", [SMALL[1], SMALL[4], LARGE])
def test_misaligned_planes_give_the_bits_of_aligned_ones(h, w):
    assert w % 4 == 0
    D, N, w_n, w_p, I = scene(h, w)
    assert torch.equal(bits(run_normals(D, JUMP)), bits(run_normals(D, JUMP, misaligned=True)))
    a, b = run_normal_loss(D, N, w_n, w_p, JUMP, 0), run_normal_loss(D, N, w_n, w_p, JUMP, 0, misaligned=True)
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))
    for flags in (R.INVERSE, R.SECOND_ORDER):
        a, b = run_smooth(D, I, w_p, 10.0, flags), run_smooth(D, I, w_p, 10.0, flags, misaligned=True)
        assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))


def test_autograd_scales_the_gradient_by_the_upstream():
    """(2.5 * loss).backward() against 2.5 times the unit-upstream gradient: both are float64 results rounded once, so they
    differ by at most the two roundings, 2^-23 of the value"""
    h, w = SMALL[3]
    D, N, w_n, w_p, I = (dev(v) for v in scene(h, w))
    for make in (lambda d: geometry.normal_loss(d, K, N, w_n, w_p, unit_range=False, convention="opengl", max_rel_jump=JUMP),
                 lambda d: geometry.depth_smoothness(d, I, w_p, space="inverse", order=2, edge_lambda=10.0)):
        d1, d2 = D.clone().requires_grad_(True), D.clone().requires_grad_(True)
        loss = make(d1)
        assert loss.terms.shape == (8,) and loss.item() == loss.terms[0].item() and loss.item() > 0
        loss.backward()
        (2.5 * make(d2)).backward()
        unit, scaled = d1.grad.double().cpu().numpy(), d2.grad.double().cpu().numpy()
        assert np.abs(unit).max() > 0
        assert np.all(np.abs(scaled - 2.5 * unit) <= 2.0 ** -23 * np.abs(2.5 * unit) + FLOOR)
        assert not bits(d2.grad)[bits(d1.grad) == 0].any()


def test_nothing_selected_gives_eight_zeros_and_a_zero_gradient():
    h, w = SMALL[2]
    D, N, w_n, w_p, I = scene(h, w)
    for terms, grad in (run_normal_loss(D, N, np.zeros_like(w_n), w_p, JUMP, 0), run_normal_loss(D, N * 0.2, w_n, None, JUMP, 0),
                        run_normal_loss(np.zeros_like(D), N, w_n, w_p, JUMP, 0), run_smooth(D, I, np.zeros_like(w_p), 10.0, 0),
                        run_smooth(np.full_like(D, np.nan), I, None, 10.0, R.SMOOTH_FLAGS_ALL)):
        assert not bits(terms).any() and not bits(grad).any()
    assert not bits(run_normals(np.zeros_like(D), 0.0)).any()


def test_work_memory_belongs_to_the_context_and_a_call_allocates_nothing():
    from taichi_3d_gaussian_splatting_amd import _native
    h, w = LARGE
    D, N, w_n, w_p, I = (dev(v) for v in scene(h, w))
    geometry.depth_smooth_forward(D, I, w_p, 10.0, 0)
    L, ctx = _native.lib(), _native.shared_ctx(D.device)
    before = L.gs_ctx_device_bytes(ctx)
    assert before >= -(-h // TH) * -(-w // TW) * 4 * 8
    free = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        terms = geometry.normal_loss_forward(D, K, N, w_n, w_p, JUMP, 0)
        geometry.normal_loss_backward(D, K, N, w_n, w_p, JUMP, 0, terms, out=torch.empty_like(D))
    torch.cuda.synchronize()
    assert L.gs_ctx_device_bytes(ctx) == before
    assert torch.cuda.mem_get_info()[0] >= free - (64 << 20)
