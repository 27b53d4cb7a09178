"""CPU: the float64 restatement of include/gs_normals.h (tests/normals_ref.py) is pinned before any GPU test trusts it: forward
and analytic backward against float64 torch autograd of the closed forms, with the axis k, the sign and the selections held
fixed by construction.  The inputs keep the restatement itself away from its discontinuities, and that is checked here:
log-scales whose smallest is at least 0.05 below the next, |m . p| / |p| >= 1e-3, rendered normals whose length is outside
[0.45, 0.55] (min_length is 0.5), depth jumps outside [0.09, 0.11] of the depth (max_rel_jump is 0.1)."""
import numpy as np
import pytest
import torch

import geometry_ref as G
import normals_ref as ref

K = (61.5, 58.25, 19.75, 14.5)              # fx, fy, cx, cy, exact in float32
H, W = 23, 29
JUMP, MIN_LENGTH = 0.1, 0.5


def _t(v):
    return torch.from_numpy(np.asarray(v, dtype=np.float64))


# ---- the normal of a Gaussian ---------------------------------------------------------------------------------------------------
def _gaussians(n=400, n_objects=2, seed=0):
    """n rows of 2 n drawn ones: those whose normal is not edge-on to the camera (the sign is a selection)"""
    pc, f, q_pc, t_pc, ids, g = _draw(2 * n, n_objects, seed)
    r = ref._rows(pc, f, q_pc, t_pc, ids)
    keep = np.flatnonzero(np.abs(r["a"]) / np.linalg.norm(r["p"], axis=1) >= 2e-3)[:n]
    assert len(keep) == n
    return pc[keep], f[keep], q_pc, t_pc, None if ids is None else ids[keep], g[keep]


def _draw(n, n_objects, seed):
    rng = np.random.default_rng(seed)
    pc = rng.uniform(-2.0, 2.0, (n, 3)).astype(np.float32)
    f = np.zeros((n, 56), dtype=np.float32)
    q = rng.normal(size=(n, 4))
    f[:, :4] = q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (n, 1))          # lengths 0.5 .. 2
    s = np.sort(rng.uniform(-4.0, -1.0, (n, 3)), axis=1)
    s[:, 1:] += 0.05                                                                                  # the smallest is 0.05 below the next
    f[:, 4:7] = np.take_along_axis(s, rng.permuted(np.tile(np.arange(3), (n, 1)), axis=1), axis=1)
    f[:, 7:] = rng.normal(size=(n, 49))
    q_pc = rng.normal(size=(n_objects, 4))
    q_pc = (q_pc / np.linalg.norm(q_pc, axis=1, keepdims=True)).astype(np.float32)
    t_pc = rng.uniform(-1.0, 1.0, (n_objects, 3)).astype(np.float32) + np.float32([0, 0, -6])
    ids = rng.integers(0, n_objects, n).astype(np.int32) if n_objects > 1 else None
    g = rng.normal(size=(n, 3)).astype(np.float32)
    return pc, f, q_pc, t_pc, ids, g


def _torch_rotation(q):
    x, y, z, w = q.unbind(-1)
    return torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                        torch.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                        torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


@pytest.mark.parametrize("n_objects", [1, 2])
def test_gaussian_normals_backward_is_the_derivative_of_the_forward(n_objects):
    pc, f, q_pc, t_pc, ids, g = _gaussians(n_objects=n_objects)
    r = ref._rows(pc, f, q_pc, t_pc, ids)
    n = len(pc)
    # away from the discontinuities: the axis choice and the sign
    s = np.sort(f[:, 4:7].astype(np.float64), axis=1)
    assert np.all(s[:, 1] - s[:, 0] >= 0.049) and r["ok"].all()
    assert np.all(np.abs(r["a"]) / np.linalg.norm(r["p"], axis=1) >= 1e-3)
    assert set(r["k"]) == {0, 1, 2} and r["flip"].any() and not r["flip"].all()
    assert np.array_equal(r["k"], np.argmin(f[:, 4:7], axis=1))

    q = _t(f[:, :4]).requires_grad_(True)
    oid = torch.zeros(n, dtype=torch.long) if ids is None else torch.from_numpy(ids.astype(np.int64))
    P = _torch_rotation(_t(q_pc))[oid]
    c = _torch_rotation(q)[torch.arange(n), :, torch.from_numpy(r["k"])]
    u = c / c.norm(dim=1, keepdim=True)
    m = torch.einsum("nij,ni->nj", P, u)
    sign = _t(np.where(r["flip"], -1.0, 1.0))[:, None]
    normals = sign * m
    (normals * _t(g)).sum().backward()

    got, magnitude = ref.gaussian_normals_forward(pc, f, q_pc, t_pc, ids)
    assert np.all(np.abs(got - normals.detach().numpy()) <= 1e-14 * magnitude)
    assert np.allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-6)                 # (the pose quaternions are unit to f32)
    # every normal faces the camera: n . p <= 0 with p the Gaussian in the camera frame
    assert np.all(np.einsum("nj,nj->n", got, r["p"]) < 0)
    grad, gmag = ref.gaussian_normals_backward(pc, f, q_pc, t_pc, ids, g)
    assert np.all(np.abs(grad[:, :4] - q.grad.numpy()) <= 1e-12 * gmag[:, :4] + 1e-300) and np.abs(grad[:, :4]).max() > 0.1
    assert not grad[:, 4:].any() and not gmag[:, 4:].any()


def test_gaussian_normals_special_rows():
    pc, f, q_pc, t_pc, ids, g = _gaussians(n=8, n_objects=1)
    f[0, 4:7] = (-2.0, -2.0, -1.0)                    # a tie of the two smallest: index 0
    f[1, 4:7] = (-1.0, -2.0, -2.0)                    # index 1
    f[2, 2] = np.nan
    pc[3, 1] = np.inf
    f[4, :4] = 0.0
    f[5, 5] = -np.inf
    f[6, :4] = (0.0, 0.5, 0.5, 0.0)                   # R00 = 1 - 2 (0.25 + 0.25) = 0, R10 = 2 (0 + 0), R20 = 2 (0 - 0): a zero column 0
    f[6, 4:7] = (-3.0, -1.0, -1.0)
    r = ref._rows(pc, f, q_pc, t_pc, ids)
    assert r["k"][0] == 0 and r["k"][1] == 1
    assert list(r["ok"]) == [True, True, False, False, False, False, False, True]
    normals, _ = ref.gaussian_normals_forward(pc, f, q_pc, t_pc, ids)
    grad, _ = ref.gaussian_normals_backward(pc, f, q_pc, t_pc, ids, g)
    for i in (2, 3, 4, 5, 6):
        assert not normals[i].any() and not grad[i].any()
    assert np.isfinite(normals).all() and np.isfinite(grad).all()


# ---- the consistency loss -------------------------------------------------------------------------------------------------------
def _pictures(seed=0):
    """a wavy depth with a step edge and holes, rendered normals near the surface's with short ones, weights with zeros"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    D = 2.0 + 0.02 * np.sin(xx / 3.0) + 0.03 * np.cos(yy / 2.0) + 0.002 * rng.uniform(-1, 1, (H, W))
    D[:, W // 2:] += 1.5
    D[3, 4] = 0.0
    D[10:12, 20] = np.nan
    D[17, 2] = np.inf
    D = D.astype(np.float32)
    R = np.stack([0.3 * rng.normal(size=(H, W)), 0.3 * rng.normal(size=(H, W)), -np.ones((H, W))], axis=2)
    R = R / np.linalg.norm(R, axis=2, keepdims=True) * rng.uniform(0.6, 1.0, (H, W, 1))
    R[rng.uniform(size=(H, W)) < 0.1] *= 0.4                                          # too short: below 0.45
    R = R.astype(np.float32)
    w_p = rng.uniform(0.2, 1.0, (H, W)).astype(np.float32)
    w_p[8, 8:12] = 0.0
    w_p[15, 3] = -1.0
    return D, R, w_p


def _check_away_from_the_thresholds(D, R):
    length = np.linalg.norm(R.astype(np.float64), axis=2)
    assert not ((length >= 0.45) & (length <= 0.55)).any() and (length < 0.45).sum() > 20
    valid = G.valid_depth(D)
    d = np.where(valid, D, 0).astype(np.float64)
    dx, dy = np.abs(G.shift(d, 0, 1) - G.shift(d, 0, -1)), np.abs(G.shift(d, 1, 0) - G.shift(d, -1, 0))
    all_valid = valid & G.shift(valid, 0, 1, False) & G.shift(valid, 0, -1, False) & G.shift(valid, 1, 0, False) & G.shift(valid, -1, 0, False)
    for v in (dx, dy):
        rel = v[all_valid] / d[all_valid]
        assert not ((rel >= 0.09) & (rel <= 0.11)).any()
    assert (dx[all_valid] / d[all_valid] > 0.11).sum() > 10                            # the step edge is there to be cut


def _autograd_consistency(D, R, w_p, jump, min_length):
    _, values, selected = ref.normal_consistency_forward(D, K, R, w_p, jump, min_length)
    w = (np.ones((H, W), np.float32) if w_p is None else G.clamp_weight(w_p)).astype(np.float64)
    sel = torch.from_numpy(selected[1:-1, 1:-1])
    Dt = _t(np.where(G.valid_depth(D), D, 0.0)).requires_grad_(True)
    Rt = _t(R).requires_grad_(True)
    l, r, u, d = Dt[1:-1, :-2], Dt[1:-1, 2:], Dt[:-2, 1:-1], Dt[2:, 1:-1]
    fx, fy, cx, cy = K
    x = torch.arange(1, W - 1, dtype=torch.float64)[None, :]
    y = torch.arange(1, H - 1, dtype=torch.float64)[:, None]
    a = lambda k: (x + k + 0.5 - cx) / fx       # noqa: E731
    b = lambda k: (y + k + 0.5 - cy) / fy       # noqa: E731
    Px = torch.stack([a(1) * r - a(-1) * l, b(0) * (r - l), (r - l) + 0 * y])
    Py = torch.stack([a(0) * (d - u), b(1) * d - b(-1) * u, (d - u) + 0 * x])
    c = torch.linalg.cross(Py, Px, dim=0)
    one = torch.ones_like(sel, dtype=torch.float64)
    n = c / torch.where(sel, (c * c).sum(0), one).sqrt()
    m = Rt[1:-1, 1:-1].permute(2, 0, 1)
    h = m / torch.where(sel, (m * m).sum(0), one).sqrt()
    cos = (n * h).sum(0)
    wt = _t(w)[1:-1, 1:-1]
    zero = torch.zeros_like(cos)
    loss = torch.where(sel, wt * (1 - cos), zero).sum() / torch.where(sel, wt, zero).sum()
    loss.backward()
    return float(loss.detach()), Dt.grad.numpy(), Rt.grad.numpy(), values


@pytest.mark.parametrize("jump,with_wp,upstream", [(JUMP, True, 1.0), (0.0, False, 1.0), (JUMP, True, -0.75)])
def test_consistency_backward_is_the_derivative_of_the_forward(jump, with_wp, upstream):
    D, R, w_p = _pictures()
    _check_away_from_the_thresholds(D, R)
    w_p = w_p if with_wp else None
    loss, grad_D_auto, grad_R_auto, values = _autograd_consistency(D, R, w_p, jump, MIN_LENGTH)
    terms, _, selected = ref.normal_consistency_forward(D, K, R, w_p, jump, MIN_LENGTH)
    assert selected.sum() > 100 and abs(loss - values["L"]) <= 1e-13 and 0 < values["L"] < 1
    assert terms[2] == selected.sum() and abs(terms[3] - values["mean_cos"]) <= 1e-6
    grad_D, mag_D, touched, grad_R, mag_R, sel = ref.normal_consistency_backward(D, K, R, w_p, jump, MIN_LENGTH, terms, upstream)
    scale = upstream * values["S_w"] / float(terms[1])                  # S_w is read as the float32 the device reads
    assert np.array_equal(sel, selected)
    assert np.all(np.abs(grad_D - grad_D_auto * scale) <= 1e-10 * mag_D + 1e-300)
    assert np.all(np.abs(grad_R - grad_R_auto * scale) <= 1e-10 * mag_R + 1e-300)
    assert np.all(grad_D[~touched] == 0) and np.all(grad_R[~selected] == 0) and np.all(mag_R[selected] > 0)
    assert np.abs(grad_R[selected]).max() > 0 and (mag_D > 0).sum() > 100
    if jump > 0:
        assert selected.sum() < ref.normal_consistency_forward(D, K, R, w_p, 0.0, MIN_LENGTH)[2].sum()      # the test cut something


def test_a_wall_seen_head_on_agrees_with_normals_that_face_the_camera():
    D = np.full((H, W), 2.5, dtype=np.float32)
    R = np.zeros((H, W, 3), dtype=np.float32)
    R[..., 2] = -0.8
    terms, values, selected = ref.normal_consistency_forward(D, K, R, None, JUMP, MIN_LENGTH)
    assert selected.sum() == (H - 2) * (W - 2) and abs(values["L"]) <= 1e-15 and abs(values["mean_cos"] - 1) <= 1e-15
    terms, values, _ = ref.normal_consistency_forward(D, K, -R, None, JUMP, MIN_LENGTH)
    assert abs(values["L"] - 2) <= 1e-15
    assert not ref.normal_consistency_forward(D, K, R * 0.5, None, JUMP, MIN_LENGTH)[0].any()                # |R| = 0.4: nothing usable
    out = ref.normal_consistency_backward(D, K, R * 0.5, None, JUMP, MIN_LENGTH, np.zeros(8, np.float32))
    assert not any(np.asarray(v).any() for v in out)
