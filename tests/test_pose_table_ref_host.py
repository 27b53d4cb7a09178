"""CPU: tests/pose_table_ref.py, the float64 restatement of include/gs_pose_table.h, against float64 torch autograd of the closed
form, its selection rule and the meeting of the series with the closed forms at the threshold."""
import numpy as np
import torch

import pose_table_ref as ref

THETAS = [0.0, 1e-9, 1e-4 * (1 - 1e-6), 1e-4 * (1 + 1e-6), 1e-3, 1.0, np.pi - 1e-3, 4.0]


def _case(V=len(THETAS), K=3, seed=0):
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=(V, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    delta = np.concatenate([axis * np.asarray(THETAS)[:V, None], rng.normal(0.0, 0.1, (V, 3))], axis=1).astype(np.float32)
    q = rng.normal(size=(V, K, 4))
    q /= np.linalg.norm(q, axis=2, keepdims=True)
    q[1] *= 1.3                                                     # a quaternion that is not of unit length, as stored
    return delta, q.astype(np.float32), rng.normal(0.0, 2.0, (V, K, 3)).astype(np.float32), rng.normal(size=(V, K, 4)).astype(np.float32), \
        rng.normal(size=(V, K, 3)).astype(np.float32)


def _torch_compose(delta, q, t):
    """the closed form in float64 torch operations; theta = 0 is never differentiated through here"""
    w, u = delta[:, :3], delta[:, 3:]
    th = w.norm(dim=1, keepdim=True)
    dq = torch.cat([w * torch.sin(th / 2) / th, torch.cos(th / 2)], dim=1)[:, None, :]
    x0, y0, z0, w0 = q.unbind(-1)
    x1, y1, z1, w1 = dq.unbind(-1)
    q_out = torch.stack([w0 * x1 + x0 * w1 + y0 * z1 - z0 * y1, w0 * y1 - x0 * z1 + y0 * w1 + z0 * x1,
                         w0 * z1 + x0 * y1 - y0 * x1 + z0 * w1, w0 * w1 - x0 * x1 - y0 * y1 - z0 * z1], dim=-1)
    R = torch.stack([1 - 2 * (y0 * y0 + z0 * z0), 2 * (x0 * y0 - w0 * z0), 2 * (x0 * z0 + w0 * y0),
                     2 * (x0 * y0 + w0 * z0), 1 - 2 * (x0 * x0 + z0 * z0), 2 * (y0 * z0 - w0 * x0),
                     2 * (x0 * z0 - w0 * y0), 2 * (y0 * z0 + w0 * x0), 1 - 2 * (x0 * x0 + y0 * y0)], dim=-1).reshape(*q.shape[:2], 3, 3)
    return q_out, t + torch.einsum("vkij,vj->vki", R, u)


def test_gradient_equals_float64_autograd_of_the_closed_form():
    delta, q, t, gq, gt = _case()
    reg = 0.25
    keep = [i for i, th in enumerate(THETAS) if th > 0.0]          # the closed form has no derivative at 0
    d = torch.tensor(delta[keep], dtype=torch.float64, requires_grad=True)
    q_out, t_out = _torch_compose(d, torch.tensor(q[keep], dtype=torch.float64), torch.tensor(t[keep], dtype=torch.float64))
    loss = (q_out * torch.tensor(gq[keep], dtype=torch.float64)).sum() + (t_out * torch.tensor(gt[keep], dtype=torch.float64)).sum() \
        + 0.5 * reg * (d ** 2).sum()
    loss.backward()
    got, _ = ref.backward64(delta, q, gq, gt, reg)
    # float64 on both sides; the closed form's (C/2 - A)/s loses digits to cancellation as s falls (1e-16 / s of them)
    np.testing.assert_allclose(got[keep], d.grad.numpy(), rtol=1e-7, atol=1e-9)
    q64, t64 = ref.compose64(delta, q, t)
    np.testing.assert_allclose(q64[keep], q_out.detach().numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(t64[keep], t_out.detach().numpy(), rtol=1e-12, atol=1e-14)
    # at zero: the limit, by central differences of the restatement itself
    z = THETAS.index(0.0)
    h = 1e-5
    for j in range(6):
        e = np.zeros((1, 6)); e[0, j] = h
        f = lambda dd: sum((a * b).sum() for a, b in zip(ref.compose64(dd, q[z:z + 1], t[z:z + 1]), (gq[z], gt[z])))
        base = np.concatenate([np.zeros(3), delta[z, 3:]])[None].astype(np.float64)
        numeric = (f(base + e) - f(base - e)) / (2 * h)
        analytic = ref.backward64(base, q[z:z + 1], gq[z:z + 1], gt[z:z + 1], 0.0)[0][0, j]
        assert abs(numeric - analytic) < 1e-8, (j, numeric, analytic)


def test_zero_delta_copies_bits_and_non_finite_poisons_its_own_view():
    _, q, t, _, _ = _case()
    q[0, 0, 0], t[0, 0, 1], t[2, 1, 2] = -0.0, -0.0, np.float32(np.nan)
    delta = np.zeros((len(THETAS), 6), dtype=np.float32)
    delta[1, 2] = -0.0
    q_out, t_out = ref.compose(delta, q, t)
    assert np.array_equal(q_out.view(np.uint32), q.view(np.uint32)) and np.array_equal(t_out.view(np.uint32), t.view(np.uint32))
    # the formulas alone would not: a quaternion of length 1.3 times (0, 0, 0, 1) is itself, but -0 + 0 is +0
    q64, _ = ref.compose64(delta, q, t)
    assert not np.array_equal(q64.astype(np.float32).view(np.uint32), q.view(np.uint32))
    delta[3, 4] = np.inf
    delta[4, 0] = np.nan
    delta[5] = [0.1, 0, 0, 0, 0, 0]
    q_out, t_out = ref.compose(delta, q, t)
    for v in (3, 4):
        assert np.isnan(q_out[v]).all() and np.isnan(t_out[v]).all()
    for v in (0, 1, 6, 7):
        assert np.array_equal(q_out[v].view(np.uint32), q[v].view(np.uint32)) and np.array_equal(t_out[v].view(np.uint32), t[v].view(np.uint32))
    assert np.isfinite(q_out[5]).all() and not np.array_equal(q_out[5], q[5]) and np.array_equal(t_out[5], t[5])


def test_series_and_closed_forms_meet_at_the_threshold():
    for s in (ref.SERIES_S, ref.SERIES_S * (1 - 1e-9), ref.SERIES_S * (1 + 1e-9), 1e-12, 1e-10):
        series, closed = ref.coefficients(s, series=True), ref.coefficients(s, series=False)
        assert abs(series[0] - closed[0]) <= 2e-16 and abs(series[1] - closed[1]) <= 2e-16, s
        # B's closed form cancels: its error is some 1e-16 / s
        assert abs(series[2] - closed[2]) <= 4e-16 / s, s
    assert ref.coefficients(0.0) == (0.5, 1.0, -1.0 / 24.0)
    assert ref.coefficients(ref.SERIES_S) == ref.coefficients(ref.SERIES_S, series=False)            # the threshold itself is closed form
    assert ref.coefficients(np.nextafter(ref.SERIES_S, 0.0)) == ref.coefficients(np.nextafter(ref.SERIES_S, 0.0), series=True)
    # the series' next terms are far below float64 at the threshold
    assert ref.SERIES_S ** 3 / 645120 < 1e-20 and ref.SERIES_S ** 3 / 46080 < 1e-20


def test_host_correction_matrix_is_the_quaternion_form():
    """write_dataset composes T * D(delta) on the host in float64: for unit quaternions it is what the kernels compose"""
    from taichi_3d_gaussian_splatting_amd import pose_table
    delta, q, t, _, _ = _case()
    for v in range(len(THETAS)):
        unit = q[v, 0].astype(np.float64)
        unit /= np.linalg.norm(unit)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = ref.rotation(unit), t[v, 0]
        want = T @ pose_table.correction_matrix(delta[v])
        q64, t64 = ref.compose64(delta[v:v + 1], unit[None, None], t[v:v + 1, :1])
        got = np.eye(4)
        got[:3, :3], got[:3, 3] = ref.rotation(q64[0, 0]), t64[0, 0]
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
        assert abs(np.linalg.det(want[:3, :3]) - 1.0) < 1e-12


def test_write_dataset_corrects_the_views_of_the_file_and_no_other(tmp_path):
    import json
    from taichi_3d_gaussian_splatting_amd import pose_table
    delta, q, t, _, _ = _case()
    records = []
    for v in range(4):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = ref.rotation(q[v, 0].astype(np.float64) / np.linalg.norm(q[v, 0].astype(np.float64))), t[v, 0]
        records.append(dict(image_path=f"images/{v}.png", T_pointcloud_camera=T.tolist(), camera_height=16, camera_width=16, extra=v))
    (tmp_path / "src.json").write_text(json.dumps(records))
    rows = torch.tensor(delta[[5, 6]])
    torch.save(dict(delta=rows, exp_avg=torch.zeros_like(rows), exp_avg_sq=torch.zeros_like(rows), steps=[1, 1],
                    image_paths=["images/1.png", "images/3.png"]), tmp_path / "poses.pt")
    assert pose_table.write_dataset(str(tmp_path / "poses.pt"), str(tmp_path / "src.json"), str(tmp_path / "dst.json")) == 2
    out = json.loads((tmp_path / "dst.json").read_text())
    assert [r["image_path"] for r in out] == [r["image_path"] for r in records] and [r["extra"] for r in out] == [0, 1, 2, 3]
    for v, row in ((0, None), (1, 5), (2, None), (3, 6)):
        base = np.asarray(records[v]["T_pointcloud_camera"])
        want = base if row is None else base @ pose_table.correction_matrix(delta[row])
        assert np.array_equal(np.asarray(out[v]["T_pointcloud_camera"]), want)
        assert (row is None) == np.array_equal(np.asarray(out[v]["T_pointcloud_camera"]), base)


def test_ulps_apart_counts_float32_steps():
    one = np.float32(1.0)
    assert ref.ulps_apart([one], [np.nextafter(one, np.float32(2))]).tolist() == [1]
    assert ref.ulps_apart([np.float32(0.0)], [np.float32(-0.0)]).tolist() == [1]
    assert ref.ulps_apart([np.nan, 1.0], [np.nan, np.nan]).tolist() == [0, 2 ** 32]
