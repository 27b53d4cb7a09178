"""CPU: the float64 restatement of include/gs_geometry.h (tests/geometry_ref.py) is pinned before any GPU test trusts it: its
analytic backward against float64 torch autograd on a differentiable restatement of the same formulas, and the closed forms a
plane has."""
import numpy as np
import pytest
import torch

import geometry_ref as ref

K = (61.5, 58.25, 19.75, 14.5)              # fx, fy, cx, cy, exact in float32
H, W = 23, 29


def _scene(seed=0):
    """a depth with holes, a prior, weights with zeros and a guide; differences of neighbouring depths are far from 0"""
    rng = np.random.default_rng(seed)
    D = rng.uniform(1.0, 4.0, (H, W)).astype(np.float32)
    D[3, 4] = 0.0
    D[10:12, 20] = np.nan
    D[17, 2] = np.inf
    N = rng.normal(size=(3, H, W))
    N = (N / np.linalg.norm(N, axis=0)).astype(np.float32)
    N[:, 6, 6] = 0.1                                                 # too short: not usable
    w_n = rng.uniform(0.2, 1.0, (H, W)).astype(np.float32)
    w_n[8, 8:12] = 0.0
    w_p = rng.uniform(0.2, 1.0, (H, W)).astype(np.float32)
    w_p[15, 3] = -1.0
    I = rng.uniform(0.0, 1.0, (3, H, W)).astype(np.float32)
    return D, N, w_n, w_p, I


def _t(v):
    return torch.from_numpy(np.asarray(v, dtype=np.float64))


def _autograd_normal_loss(D, N, w_n, w_p, jump, flags):
    """the loss of the header in torch float64 on the interior pixels, the selection (from the restatement) held fixed"""
    _, values, selected = ref.normal_loss_forward(D, K, N, w_n, w_p, jump, flags)
    _, h = ref.decode_prior(N, flags)
    w = (ref.clamp_weight(w_n) * (np.float32(1) if w_p is None else ref.clamp_weight(w_p))).astype(np.float64)     # one f32 multiply
    sel = torch.from_numpy(selected[1:-1, 1:-1])
    Dt = _t(np.where(ref.valid_depth(D), D, 0.0)).requires_grad_(True)
    l, r, u, d = Dt[1:-1, :-2], Dt[1:-1, 2:], Dt[:-2, 1:-1], Dt[2:, 1:-1]
    fx, fy, cx, cy = K
    x = torch.arange(1, W - 1, dtype=torch.float64)[None, :]
    y = torch.arange(1, H - 1, dtype=torch.float64)[:, None]
    a = lambda k: (x + k + 0.5 - cx) / fx       # noqa: E731
    b = lambda k: (y + k + 0.5 - cy) / fy       # noqa: E731
    Px = torch.stack([a(1) * r - a(-1) * l, b(0) * (r - l), (r - l) + 0 * y])
    Py = torch.stack([a(0) * (d - u), b(1) * d - b(-1) * u, (d - u) + 0 * x])
    c = torch.linalg.cross(Py, Px, dim=0)
    q = torch.where(sel, (c * c).sum(0), torch.ones_like(sel, dtype=torch.float64))
    n = c / q.sqrt()
    cos = (n * _t(h)[:, 1:-1, 1:-1]).sum(0)
    wt = _t(w)[1:-1, 1:-1]
    zero = torch.zeros_like(cos)
    loss = torch.where(sel, wt * (1 - cos), zero).sum() / torch.where(sel, wt, zero).sum()
    loss.backward()
    return float(loss.detach()), Dt.grad.numpy(), values


@pytest.mark.parametrize("flags,jump,with_wp", [(0, 0.0, True), (ref.PRIOR_FLIP_YZ, 0.0, False), (0, 0.9, True)])
def test_normal_backward_is_the_derivative_of_the_forward(flags, jump, with_wp):
    D, N, w_n, w_p, _ = _scene()
    w_p = w_p if with_wp else None
    loss, grad_auto, values = _autograd_normal_loss(D, N, w_n, w_p, jump, flags)
    terms, _, selected = ref.normal_loss_forward(D, K, N, w_n, w_p, jump, flags)
    assert selected.sum() > 100 and abs(loss - values["L"]) <= 1e-13
    # the restatement reads S_w as a float32, as the device does: compare at that value
    grad, magnitude, _ = ref.normal_loss_backward(D, K, N, w_n, w_p, jump, flags, terms)
    scale = values["S_w"] / float(terms[1])
    assert np.all(np.abs(grad - grad_auto * scale) <= 1e-10 * magnitude + 1e-300)
    assert np.all(grad[magnitude == 0] == 0) and (magnitude > 0).sum() > 100
    if jump > 0:
        assert selected.sum() < ref.normal_loss_forward(D, K, N, w_n, w_p, 0.0, flags)[2].sum()      # the test cut something


def _autograd_smooth(D, I, w_p, edge_lambda, flags):
    fields = ref.smooth_term_fields(D, I, w_p, edge_lambda, flags)
    valid = ref.valid_depth(D)
    Dt = _t(np.where(valid, D, 1.0)).requires_grad_(True)
    x = 1.0 / Dt if flags & ref.INVERSE else Dt
    pad = torch.nn.functional.pad(x, (2, 2, 2, 2))
    at = lambda dy, dx: pad[2 + dy:2 + dy + H, 2 + dx:2 + dx + W]       # noqa: E731
    num, den = 0.0, 0.0
    for t in fields:
        r = sum(coefficient * at(dy, dx) for (dy, dx), coefficient in t["members"])
        sel = torch.from_numpy(t["selected"])
        num = num + torch.where(sel, _t(t["we"]) * r.abs(), torch.zeros_like(r)).sum()
        den = den + _t(t["w"])[sel].sum()
    loss = num / den
    loss.backward()
    return float(loss.detach()), np.where(valid, Dt.grad.numpy(), 0.0)


@pytest.mark.parametrize("flags", [0, ref.INVERSE, ref.SECOND_ORDER, ref.INVERSE | ref.SECOND_ORDER])
@pytest.mark.parametrize("guided", [True, False])
def test_smoothness_backward_is_the_derivative_of_the_forward(flags, guided):
    D, _, _, w_p, I = _scene(1)
    I = I if guided else None
    loss, grad_auto = _autograd_smooth(D, I, w_p, 10.0, flags)
    terms, values = ref.depth_smooth_forward(D, I, w_p, 10.0, flags)
    assert values["count"] > 500 and abs(loss - values["L"]) <= 1e-13 * max(1.0, abs(loss))
    grad, magnitude, _ = ref.depth_smooth_backward(D, I, w_p, 10.0, flags, terms)
    scale = values["S_w"] / float(terms[1])
    assert np.all(np.abs(grad - grad_auto * scale) <= 1e-10 * magnitude + 1e-300)
    assert np.all(grad[magnitude == 0] == 0)


def _plane_depth(normal, offset):
    """float64 z-depth of the plane normal . P = offset seen through K, and its unit normal facing the camera"""
    fx, fy, cx, cy = K
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    rays = np.stack([(xx + 0.5 - cx) / fx, (yy + 0.5 - cy) / fy, np.ones_like(xx)])
    normal = np.asarray(normal, dtype=np.float64)
    normal = normal / np.linalg.norm(normal)
    D = offset / (normal[:, None, None] * rays).sum(0)
    assert D.min() > 0
    return D, (-normal if normal[2] > 0 else normal)


@pytest.mark.parametrize("normal", [(0.0, 0.0, 1.0), (0.3, -0.2, 1.0), (-0.5, 0.4, 0.8)])
def test_the_depth_of_a_plane_gives_the_planes_normal_at_every_interior_pixel(normal):
    D, facing = _plane_depth(normal, 2.5)
    n, _ = ref.depth_normals(D, K)                       # float64 depth: the back-projected points lie on the plane
    interior = np.zeros((H, W), dtype=bool)
    interior[1:-1, 1:-1] = True
    assert np.all(np.abs(n[:, interior] - facing[:, None]) <= 1e-12)
    assert np.all(n[:, ~interior] == 0)
    if normal == (0.0, 0.0, 1.0):
        assert np.all(n[2, interior] == -1.0)            # fronto-parallel: towards the camera


def test_second_order_smoothness_of_a_plane_is_zero():
    # a depth that is affine in the pixel coordinates costs nothing in depth space ...
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    affine = 2.0 + 0.125 * xx + 0.0625 * yy
    _, values = ref.depth_smooth_forward(affine, None, None, 10.0, ref.SECOND_ORDER)
    assert values["count"] == (W - 2) * H + (H - 2) * W and values["L"] <= 1e-15
    assert ref.depth_smooth_forward(affine, None, None, 10.0, 0)[1]["L"] > 0.05
    # ... and the z-depth of a slanted plane seen through a pinhole is affine in INVERSE depth: it costs nothing there, and
    # something in depth space
    D, _ = _plane_depth((0.3, -0.2, 1.0), 2.5)
    _, values = ref.depth_smooth_forward(D, None, None, 10.0, ref.SECOND_ORDER | ref.INVERSE)
    assert values["count"] == (W - 2) * H + (H - 2) * W and values["L"] <= 1e-15
    assert ref.depth_smooth_forward(D, None, None, 10.0, ref.SECOND_ORDER)[1]["L"] > 1e-8


def test_opengl_equals_opencv_on_a_prior_with_y_and_z_negated():
    D, N, w_n, w_p, _ = _scene(2)
    flipped = N * np.array([1.0, -1.0, -1.0], dtype=np.float32)[:, None, None]
    a = ref.normal_loss_forward(D, K, N, w_n, w_p, 0.0, 0)
    b = ref.normal_loss_forward(D, K, flipped, w_n, w_p, 0.0, ref.PRIOR_FLIP_YZ)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    ga = ref.normal_loss_backward(D, K, N, w_n, w_p, 0.0, 0, a[0])[0]
    gb = ref.normal_loss_backward(D, K, flipped, w_n, w_p, 0.0, ref.PRIOR_FLIP_YZ, b[0])[0]
    assert np.array_equal(ga, gb)
    # the unit-range encoding decodes to the same prior
    coded = ((N.astype(np.float64) + 1.0) / 2.0).astype(np.float32)
    c = ref.normal_loss_forward(D, K, coded, w_n, w_p, 0.0, ref.PRIOR_UNIT_RANGE)
    assert np.array_equal(a[2], c[2]) and abs(c[1]["L"] - a[1]["L"]) <= 1e-6
