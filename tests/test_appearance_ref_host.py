"""CPU: the numpy restatement of include/gs_appearance.h (appearance_ref.py) against torch float64 autograd, and the fit's
solve (appearance.solve_affine) on the reference's moments.  This pins the yardstick of the GPU tests."""
import numpy as np
import pytest
import torch

import appearance_ref as ref


def _case(seed, H=9, W=7):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 1.0, (3, H, W)).astype(np.float32)
    g = rng.normal(0.0, 1.0, (3, H, W)).astype(np.float32)
    M = (np.eye(3, 4) + rng.normal(0.0, 0.2, (3, 4))).astype(np.float32).reshape(12)
    return x, g, M


def _einsum_apply(x, M):
    M = M.reshape(3, 4)
    return torch.einsum("ij,jhw->ihw", M[:, :3], x) + M[:, 3, None, None]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_apply_and_gradients_agree_with_float64_autograd(seed):
    x, g, M = _case(seed)
    g[:, 2, 3] = 0.0                                    # one pixel that is not selected
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    Mt = torch.tensor(M, dtype=torch.float64, requires_grad=True)
    c = _einsum_apply(xt, Mt)
    c.backward(torch.tensor(g, dtype=torch.float64))
    # f32 with the stated order against float64: a few f32 ulp of the magnitudes (|A| <= 2, |x| <= 1, |g| <= 5)
    assert np.abs(ref.apply(x, M) - c.detach().numpy()).max() < 1e-6
    assert np.abs(ref.grad_image(g, M) - xt.grad.numpy()).max() < 4e-6
    assert ref.apply(x, M).dtype == np.float32 and ref.grad_image(g, M).dtype == np.float32
    assert np.all(ref.grad_image(g, M)[:, 2, 3] == 0.0)
    value, magnitude = ref.grad_transform(x, g)
    assert np.abs(value - Mt.grad.numpy()).max() < 1e-12 * max(1.0, magnitude.max())
    assert np.all(magnitude >= np.abs(value))


def test_the_operation_order_is_the_headers():
    """a case where the order of the three additions shows in f32: 1 + 2^-24 + 2^-24"""
    t = np.float32(2.0 ** -24)
    x = np.array([1.0, 1.0, 1.0], dtype=np.float32).reshape(3, 1, 1)
    M = np.array([1, t, t, 0, t, t, 1, 0, 0, 0, 0, 0], dtype=np.float32)
    c = ref.apply(x, M)
    assert c[0, 0, 0] == np.float32(1.0)                                # (1 + t) rounds to 1, then again
    assert c[1, 0, 0] == np.float32(1.0) + np.float32(2.0 ** -23)       # (t + t) + 1 keeps the bit
    g = np.array([1.0, 1.0, 1.0], dtype=np.float32).reshape(3, 1, 1)
    Mg = np.array([1, t, 0, 0, t, t, 0, 0, t, 1, 0, 0], dtype=np.float32)
    gi = ref.grad_image(g, Mg)
    assert gi[0, 0, 0] == np.float32(1.0) and gi[1, 0, 0] == np.float32(1.0) + np.float32(2.0 ** -23)


def test_selection_keeps_nan_out_of_every_sum():
    x, g, M = _case(3)
    g[:, 1, 1] = 0.0
    g[:, 4, 2] = [0.0, -0.0, 0.0]
    x[:, 1, 1] = [np.nan, np.inf, -np.inf]
    x[:, 4, 2] = np.nan
    value, magnitude = ref.grad_transform(x, g)
    assert np.all(np.isfinite(value)) and np.all(np.isfinite(magnitude))
    gi = ref.grad_image(g, M)
    assert np.all(np.isfinite(gi)) and np.all(gi[:, 1, 1] == 0.0) and np.all(gi[:, 4, 2] == 0.0)
    clean = x.copy()
    clean[:, 1, 1] = 0.0
    clean[:, 4, 2] = 0.0
    assert np.array_equal(ref.grad_transform(clean, g)[0], value)
    # all-zero upstream: twelve exact zeros
    assert np.array_equal(ref.grad_transform(x, np.zeros_like(g))[0], np.zeros(12))
    # a NaN upstream is selected: it poisons, as multiplication would
    g[0, 0, 0] = np.nan
    assert np.isnan(ref.grad_transform(x, g)[0][0])


def test_moments_are_the_normal_equations():
    x, _, _ = _case(4, 12, 10)
    y, _, _ = _case(5, 12, 10)
    rng = np.random.default_rng(6)
    w = rng.uniform(-0.5, 1.0, (12, 10)).astype(np.float32)
    w[0, 0], w[3, 3] = np.nan, 0.0
    x[:, 0, 0] = np.nan                                 # under a NaN weight: selected out
    y[:, 3, 3] = np.inf                                 # under a zero weight
    value, magnitude = ref.moments(x, y, w)
    assert np.all(np.isfinite(value)) and value.shape == (23,) and np.all(magnitude >= np.abs(value) - 1e-12)
    we = torch.tensor(ref.effective_weight(w, (12, 10)))
    xs, ys = torch.tensor(np.nan_to_num(x, nan=0.0), dtype=torch.float64), torch.tensor(np.nan_to_num(y, posinf=0.0), dtype=torch.float64)
    u = torch.cat([xs, torch.ones(1, 12, 10, dtype=torch.float64)])
    G = torch.einsum("hw,ihw,jhw->ij", we, u, u).numpy()
    B = torch.einsum("hw,ihw,jhw->ij", we, ys, u).numpy()
    assert np.allclose([G[i, j] for i, j in ref.UPPER_TRIANGLE], value[:10], rtol=1e-13, atol=1e-13)
    assert np.allclose(B.reshape(12), value[10:22], rtol=1e-13, atol=1e-13)
    assert np.isclose(value[22], float(we.sum()), rtol=1e-14) and value[9] == value[22]
    # None is a weight of one everywhere
    ones = ref.moments(np.nan_to_num(x), np.nan_to_num(y, posinf=0.0), None)[0]
    assert ones[22] == 120.0
    # an empty mask: zeros
    assert np.array_equal(ref.moments(x, y, np.full((12, 10), -1.0, dtype=np.float32))[0], np.zeros(23))


def test_fit_recovers_an_exact_affine_relation_to_float64_accuracy():
    from taichi_3d_gaussian_splatting_amd import appearance
    rng = np.random.default_rng(7)
    x = rng.uniform(0.0, 1.0, (3, 16, 12)).astype(np.float32)
    M = np.eye(3, 4) * [[1.1], [0.9], [1.05]] + rng.normal(0.0, 0.05, (3, 4))
    M = np.round(M * 256.0) / 256.0                     # so that y = M u is exact in f32: 8 fractional bits on 24-bit inputs
    x = (np.round(x * 4096.0) / 4096.0).astype(np.float32)
    y64 = np.einsum("ij,jhw->ihw", M[:, :3], x.astype(np.float64)) + M[:, 3, None, None]
    y = y64.astype(np.float32)
    assert np.array_equal(y.astype(np.float64), y64)
    w = rng.uniform(0.1, 1.0, (16, 12)).astype(np.float32)
    for weight in (None, w):
        m, _ = ref.moments(x, y, weight)
        fit = appearance.solve_affine(m)
        assert fit.dtype == np.float64 and np.abs(fit - M.reshape(12)).max() < 1e-11
        assert np.array_equal(fit, ref.solve_affine(m))


def test_fit_is_the_identity_for_a_singular_system():
    from taichi_3d_gaussian_splatting_amd import appearance
    identity = np.array(appearance.IDENTITY)
    assert np.array_equal(identity, ref.IDENTITY)
    y = _case(8)[0]
    constant = np.full_like(y, 0.25)                    # a constant image: u spans one direction only
    grey = np.broadcast_to(_case(9)[0][:1], y.shape).copy()     # three equal channels: rank 2
    for x in (constant, grey):
        m, _ = ref.moments(x, y)
        assert np.array_equal(appearance.solve_affine(m), identity) and np.array_equal(ref.solve_affine(m), identity)
    assert np.array_equal(appearance.solve_affine(np.zeros(23)), identity)                        # sum w == 0
    bad = ref.moments(_case(10)[0], y)[0]
    bad[4] = np.nan
    assert np.array_equal(appearance.solve_affine(bad), identity)


def test_learning_rate_schedule():
    from taichi_3d_gaussian_splatting_amd.appearance import AppearanceConfig
    cfg = AppearanceConfig(num_iterations=1000)
    assert cfg.lr_at(0) == pytest.approx(0.01) and cfg.lr_at(1000) == pytest.approx(0.001) and cfg.lr_at(5000) == pytest.approx(0.001)
    assert cfg.lr_at(500) == pytest.approx((0.01 * 0.001) ** 0.5)
    assert all(cfg.lr_at(i) == pytest.approx(ref.lr_at(i, num_iterations=1000)) for i in (0, 1, 250, 999))
    assert AppearanceConfig().lr_at(123) == 0.01 and (AppearanceConfig().lr, AppearanceConfig().lr_final) == (0.01, 0.001)
    from taichi_3d_gaussian_splatting_amd.optim import FusedAdam
    import inspect
    assert AppearanceConfig().eps == inspect.signature(FusedAdam.__init__).parameters["eps"].default
    assert tuple(AppearanceConfig().betas) == inspect.signature(FusedAdam.__init__).parameters["betas"].default
