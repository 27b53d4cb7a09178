"""CPU: tests/filter3d_ref.py, the numpy restatement of include/gs_filter3d.h, against independent forms: the rate against a
float64 brute force, the transform against logit(sigmoid(a) sqrt(det S^2 / det(S^2 + v))) in float64 torch, its gradient against
float64 autograd of that closed form, and the identity of a zero filter."""
import numpy as np
import torch

import filter3d_ref as ref

F = np.float32
W, H, NEAR, MARGIN = 96, 64, 0.8, 0.15


def cameras(n_views, rng, fx=80.0, fy=70.0):
    """n_views (16,) rows looking at the origin from a ring of radius about 4"""
    rows = []
    for i in range(n_views):
        angle = 2 * np.pi * i / max(n_views, 1) + rng.uniform(-0.1, 0.1)
        centre = np.array([4.0 * np.sin(angle), rng.uniform(-0.5, 0.5), -4.0 * np.cos(angle)])
        z = -centre / np.linalg.norm(centre)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        R = np.stack([x, y, z])                          # camera from point cloud
        rows.append(np.concatenate([R.reshape(9), -R @ centre, [fx * (1 + 0.1 * i), fy, W / 2 + 0.3, H / 2 - 0.2]]))
    return np.asarray(rows, dtype=F).reshape(-1, 16)


def brute_force(pc, views):
    """float64: -> (seen (N,V), rate of every pair (N,V), the smallest distance of any comparison from its threshold (N,V),
    relative to the threshold's scale)"""
    pc, views = pc.astype(np.float64), views.astype(np.float64)
    n, v = pc.shape[0], views.shape[0]
    seen, rates, slack = np.zeros((n, v), bool), np.zeros((n, v)), np.full((n, v), np.inf)
    for j, w in enumerate(views):
        p = pc @ w[:9].reshape(3, 3).T + w[9:12]
        with np.errstate(all="ignore"):
            u, vv = w[12] * p[:, 0] / p[:, 2] + w[14], w[13] * p[:, 1] / p[:, 2] + w[15]
        seen[:, j] = (p[:, 2] > NEAR) & (-MARGIN * W <= u) & (u <= (1 + MARGIN) * W) & (-MARGIN * H <= vv) & (vv <= (1 + MARGIN) * H)
        with np.errstate(all="ignore"):
            rates[:, j] = max(w[12], w[13]) / p[:, 2]
        gaps = [np.abs(p[:, 2] - NEAR), np.abs(u + MARGIN * W) / W, np.abs(u - (1 + MARGIN) * W) / W, np.abs(vv + MARGIN * H) / H,
                np.abs(vv - (1 + MARGIN) * H) / H]
        # behind the camera the projection means nothing: only the depth decides
        slack[:, j] = np.where(p[:, 2] > NEAR, np.min(gaps, axis=0), gaps[0])
    return seen, rates, slack


def test_rate_equals_a_float64_brute_force_away_from_the_thresholds():
    rng = np.random.default_rng(0)
    views = cameras(7, rng)
    pc = rng.uniform(-8.0, 8.0, (4000, 3)).astype(F)
    mask = (rng.uniform(size=4000) < 0.1).astype(np.int8)
    seen, rates, slack = brute_force(pc, views)
    clear = (slack > 1e-4).all(axis=1)                   # f32 error of u is about 1e-6 of W: every comparison is decided
    assert clear.mean() > 0.99
    any_seen = seen.any(axis=1)
    assert 0.2 < any_seen[mask == 0].mean() < 0.95, "some valid rows must be seen by no view"
    got = ref.rate(pc, mask, views, W, H, NEAR, MARGIN)
    assert got.dtype == F and got.shape == (4000,)
    assert np.all(np.isinf(got[mask == 1]))
    want = np.where(seen, rates, 0.0).max(axis=1)
    rows = clear & (mask == 0) & any_seen
    assert rows.sum() > 500
    assert np.abs(got[rows] / want[rows] - 1.0).max() < 1e-5
    # a row no view sees takes the smallest rate of the seen rows; with fx != fy the larger focal length counts
    smallest = got[(mask == 0) & any_seen & clear].min()
    unseen = clear & (mask == 0) & ~any_seen
    if clear.all():
        assert np.all(got[unseen] == got[(mask == 0) & any_seen].min())
    assert np.all(got[unseen] <= smallest)
    assert views[0, 12] > views[0, 13]


def test_rate_of_nothing_seen_no_view_and_invalid_rows():
    rng = np.random.default_rng(1)
    views = cameras(3, rng)
    behind = np.array([[0.0, 500.0, 0.0], [0.0, -500.0, 1.0], [np.nan, 0.0, 0.0]], dtype=F)       # far above, far below, nowhere
    assert np.all(np.isinf(ref.rate(behind, np.zeros(3, np.int8), views, W, H, NEAR, MARGIN)))
    pc = rng.uniform(-1, 1, (5, 3)).astype(F)
    assert np.all(np.isinf(ref.rate(pc, np.zeros(5, np.int8), views[:0], W, H, NEAR, MARGIN)))
    got = ref.rate(pc, np.array([0, 1, 0, 1, 0], np.int8), views, W, H, NEAR, MARGIN)
    assert np.isinf(got).tolist() == [False, True, False, True, False]
    assert ref.rate(pc[:0], np.zeros(0, np.int8), views, W, H, NEAR, MARGIN).shape == (0,)


def rows(n, rng):
    feat = rng.normal(0.0, 1.0, (n, 56)).astype(F)
    feat[:, 4:7] = rng.uniform(-5.0, 2.0, (n, 3))
    feat[:, 7] = rng.uniform(-10.0, 10.0, n)
    f = np.exp(rng.uniform(np.log(1e-3), np.log(10.0), n))
    k = 0.5
    rate = (k / f).astype(F)
    return feat, rate, k


def closed_form(features, f):
    """torch float64: (N,56) -> the filtered log-scales and logit as the definition has them"""
    v = (f * f)[:, None]
    s2 = torch.exp(2.0 * features[:, 4:7])
    ls = 0.5 * torch.log(s2 + v)
    c = torch.sqrt(torch.prod(s2, dim=1) / torch.prod(s2 + v, dim=1))
    p = torch.sigmoid(features[:, 7]) * c
    return ls, torch.log(p / (1.0 - p))


def test_apply_equals_the_closed_form_in_float64():
    rng = np.random.default_rng(2)
    feat, rate, k = rows(3000, rng)
    out, after = ref.apply(feat, rate, k)
    assert out.dtype == F and after.dtype == F
    f = torch.from_numpy(ref.filter_width(rate, k).astype(np.float64))
    ls, logit = closed_form(torch.from_numpy(feat.astype(np.float64)), f)
    # both are float64 evaluations rounded (the reference) or not (the closed form): half an ulp of float32, and what the
    # closed form's 1 - p loses, 2^-52 / (1 - p) relative with 1 - p > 4e-5 here
    assert np.all(np.abs(out[:, 4:7] - ls.numpy()) <= 0.5 * ref.ulp_of(ls.numpy()) + 1e-12)
    assert np.all(np.abs(out[:, 7] - logit.numpy()) <= 0.5 * ref.ulp_of(logit.numpy()) + 1e-9 * np.abs(logit.numpy()) + 1e-12)
    assert np.array_equal(out[:, 8:].view(np.int32), feat[:, 8:].view(np.int32))
    q = ref.normalised_quaternions(feat[:, :4])
    assert np.array_equal(out[:, :4].view(np.int32), q.view(np.int32)) and np.array_equal(after[:, :4].view(np.int32), q.view(np.int32))
    assert np.array_equal(after[:, 4:].view(np.int32), feat[:, 4:].view(np.int32))
    assert np.abs(np.linalg.norm(q.astype(np.float64), axis=1) - 1.0).max() < 2e-7
    # the filter only widens and only dims
    assert np.all(out[:, 4:7] >= feat[:, 4:7]) and np.all(out[:, 7] <= feat[:, 7])


def test_apply_does_not_saturate_where_sigmoid_rounds_to_one():
    feat = np.zeros((4, 56), dtype=F)
    feat[:, 3] = 1.0
    feat[:, 4:7] = -2.0
    feat[:, 7] = [20.0, 30.0, 40.0, -20.0]
    rate = np.full(4, 10.0, dtype=F)
    out, _ = ref.apply(feat, rate, 1.0)                  # f = 0.1, s = 0.135
    assert np.all(np.isfinite(out))
    s2, v = np.exp(-4.0), 0.01
    c = (s2 / (s2 + v)) ** 1.5
    # sigmoid(a) = 1 to 1e-9: the logit of c itself; at -20 the product: a + log c
    assert np.allclose(out[:3, 7], np.log(c / (1 - c)), rtol=1e-6)
    assert np.isclose(out[3, 7], -20.0 + np.log(c), rtol=1e-6)


def test_backward_equals_float64_autograd_of_the_closed_form():
    rng = np.random.default_rng(3)
    feat, rate, k = rows(2000, rng)
    grad = rng.normal(0.0, 1.0, feat.shape).astype(F)
    grad[::7, 7] = 0.0
    grad[::5, 4:7] = 0.0
    x = torch.from_numpy(feat.astype(np.float64)).requires_grad_(True)
    f = torch.from_numpy(ref.filter_width(rate, k).astype(np.float64))
    ls, logit = closed_form(x, f)
    g = torch.from_numpy(grad.astype(np.float64))
    ((ls * g[:, 4:7]).sum() + (logit * g[:, 7]).sum()).backward()
    got64, mag = ref.apply_backward_f64(grad, feat, rate, k)
    got = ref.apply_backward(grad, feat, rate, k)
    want = x.grad.numpy()
    # 1 - r_j cancels where the filter is small beside the scale: it is at least v / (s + v) >= 1e-6 / e^4 = 1.8e-8 here, so
    # its relative error in float64 is at most 2^-52 / 1.8e-8 = 1.2e-8, in the reference and in autograd's own form alike
    assert np.all(np.abs(got64[:, 4:8] - want[:, 4:8]) <= 1e-7 * mag[:, 4:8] + 1e-300)
    assert np.all(np.abs(got[:, 4:8] - want[:, 4:8]) <= 0.5 * ref.ulp_of(want[:, 4:8]) + 1e-7 * mag[:, 4:8] + 1e-300)
    keep = [c for c in range(56) if c not in (4, 5, 6, 7)]
    assert np.array_equal(got[:, keep].view(np.int32), grad[:, keep].view(np.int32))
    # zero upstream values give exact zeros, whatever the row holds
    zeros = ref.apply_backward(np.zeros_like(grad), feat, rate, k)
    assert not zeros.any() and not np.signbit(zeros).any()
    both = (grad[:, 7] == 0) & (grad[:, 4] == 0)
    assert both.any() and not got[both, 4].any()


def test_a_zero_filter_is_the_identity():
    rng = np.random.default_rng(4)
    feat, rate, _ = rows(50, rng)
    grad = rng.normal(0.0, 1.0, feat.shape).astype(F)
    for r, k in ((rate, 0.0), (np.full(50, np.inf, dtype=F), 0.5), (np.full(50, np.nan, dtype=F), 0.5)):
        out, after = ref.apply(feat, r, k)
        assert np.array_equal(out.view(np.int32), feat.view(np.int32))          # the quaternion too: the row is not touched
        assert np.array_equal(after.view(np.int32), feat.view(np.int32))
        assert np.array_equal(ref.apply_backward(grad, feat, r, k).view(np.int32), grad.view(np.int32))
    assert ref.filter_k(0.2, 4) == float(np.sqrt(F(0.2)) * F(4.0))
    assert ref.ulp_distance(F(1.0), np.nextafter(F(1.0), F(2.0))) == 1 and ref.ulp_distance(F(-0.0), F(0.0)) == 0
