"""CPU: tests/bilateral_ref.py, the numpy restatement of include/gs_bilateral.h, pinned before any GPU test trusts it: its
float64 form against torch's grid_sample (forward and autograd), the guide's gradient against central differences, a constant
grid against the affine apply, the total variation against float64 autograd, and its f32 ordered sums against its float64 ones."""
import numpy as np
import pytest
import torch

import appearance_ref
import bilateral_ref as ref

GRIDS = [(2, 2, 2), (3, 5, 4), (16, 16, 8)]                # (Gx, Gy, L)
IMAGES = [(1, 1), (1, 7), (37, 53)]                         # (H, W)


def _case(Gx, Gy, L, H, W, seed=0):
    rng = np.random.default_rng(seed + 1000 * Gx + 10 * L + H)
    image = rng.uniform(-0.2, 1.3, (3, H, W)).astype(np.float32)          # some luminances clamp on either side
    grid = (ref.identity_grid(Gx, Gy, L) + rng.normal(0, 0.3, (Gy, Gx, L, 12))).astype(np.float32)
    upstream = rng.normal(0, 1, (3, H, W)).astype(np.float32)
    return image, grid, upstream


@pytest.mark.parametrize("dims", GRIDS)
@pytest.mark.parametrize("size", IMAGES)
def test_float64_form_equals_grid_sample_forward_and_autograd(dims, size):
    Gx, Gy, L = dims
    H, W = size
    image, grid, upstream = _case(Gx, Gy, L, H, W)
    ti = torch.tensor(image, dtype=torch.float64, requires_grad=True)
    tg = torch.tensor(grid, dtype=torch.float64, requires_grad=True)
    out = ref.torch_slice(ti, tg)
    out.backward(torch.tensor(upstream, dtype=torch.float64))
    assert np.allclose(ref.slice(image, grid, np.float64), out.detach().numpy(), rtol=1e-12, atol=1e-12)
    assert np.allclose(ref.grad_image(image, upstream, grid, np.float64), ti.grad.numpy(), rtol=1e-11, atol=1e-11)
    value, magnitude = ref.grad_grid64(image, upstream, Gx, Gy, L)
    # (absolute part: grid_sample forms its coordinates from [-1, 1], so a weight that is exactly 0 here is ~1e-16 there)
    assert np.all(np.abs(value - tg.grad.numpy()) <= 1e-13 * magnitude + 1e-12)
    # and the f32 restatement is the same mathematics: forward within f32 rounding of the float64 form
    assert np.allclose(ref.slice(image, grid), ref.slice(image, grid, np.float64), rtol=0, atol=2e-5)


def test_guide_gradient_by_central_differences():
    Gx, Gy, L, H, W = 3, 5, 4, 9, 11
    image, grid, upstream = _case(Gx, Gy, L, H, W, seed=3)
    x64 = image.astype(np.float64)
    _, tz, inside = ref.level(x64, L, np.float64)
    smooth = inside & (tz > 0.05) & (tz < 0.95)                  # away from the kinks of the guide
    assert smooth.sum() > 20
    analytic = ref.grad_image(image, upstream, grid, np.float64)
    without_guide = np.stack([sum(ref.transform(image, grid, np.float64)[0][4 * i + j] * upstream[i] for i in range(3)) for j in range(3)])
    h = 1e-6
    guide_term_seen = 0.0
    for j in range(3):
        plus, minus = x64.copy(), x64.copy()
        plus[j] += h
        minus[j] -= h
        numeric = ((ref.slice(plus, grid, np.float64) - ref.slice(minus, grid, np.float64)) * upstream).sum(0) / (2 * h)
        assert np.allclose(numeric[smooth], analytic[j][smooth], rtol=1e-6, atol=1e-7)
        guide_term_seen = max(guide_term_seen, float(np.abs(analytic[j] - without_guide[j])[smooth].max()))
    assert guide_term_seen > 1e-2                                # the term through the luminance is there and is not small


def test_constant_grid_is_the_affine_apply_exactly():
    rng = np.random.default_rng(5)
    transform = rng.normal(0, 1, 12).astype(np.float32)
    for (Gx, Gy, L), (H, W) in zip(GRIDS, IMAGES):
        image, _, upstream = _case(Gx, Gy, L, H, W, seed=7)
        grid = np.tile(transform, (Gy, Gx, L, 1))
        assert np.array_equal(ref.slice(image, grid), appearance_ref.apply(image, transform))
        # no level differs from the next: the guide's term vanishes and the image's gradient is the affine one
        assert np.array_equal(ref.grad_image(image, upstream, grid), appearance_ref.grad_image(upstream, transform))


def _torch_tv(grid):
    """gsplat's total_variation_loss of one grid (Gy,Gx,L,12): the mean of the squared neighbour differences, summed over the axes"""
    return sum((torch.diff(grid, dim=a) ** 2).mean() for a in (1, 0, 2))


@pytest.mark.parametrize("dims", GRIDS + [(64, 64, 8)])
def test_total_variation_and_its_gradient(dims):
    Gx, Gy, L = dims
    rng = np.random.default_rng(Gx)
    grid = (ref.identity_grid(Gx, Gy, L) + rng.normal(0, 0.3, (Gy, Gx, L, 12))).astype(np.float32)
    tg = torch.tensor(grid, dtype=torch.float64, requires_grad=True)
    value = _torch_tv(tg)
    value.backward()
    v64, g64 = ref.tv64(grid)
    assert abs(v64 - value.item()) <= 1e-12 * abs(value.item())
    assert np.allclose(g64, tg.grad.numpy(), rtol=1e-12, atol=1e-15)
    # the ordered restatement: float64 sums of f32 differences, one rounding to f32 at the end
    assert abs(float(ref.tv(grid)) - v64) <= 1e-6 * v64
    before = rng.normal(0, 1, grid.shape).astype(np.float32)
    after = ref.tv_add_grad(grid, 10.0, before)
    assert np.allclose(after, before + 10.0 * g64, rtol=0, atol=1e-6 + 1e-6 * np.abs(before))
    assert ref.tv(ref.identity_grid(Gx, Gy, L)) == 0.0
    assert np.array_equal(ref.tv_add_grad(ref.identity_grid(Gx, Gy, L), 10.0, before), before)


@pytest.mark.parametrize("dims,size", [((2, 2, 2), (37, 53)), ((3, 5, 4), (37, 53)), ((16, 16, 8), (37, 53)), ((16, 16, 8), (8, 8)), ((16, 16, 8), (4, 4)), ((3, 5, 4), (1, 7))])
def test_ordered_grid_gradient_is_the_float64_sum(dims, size):
    Gx, Gy, L = dims
    H, W = size
    image, _, upstream = _case(Gx, Gy, L, H, W, seed=11)
    upstream[:, ::3, ::2] = 0.0                                  # pixels that are not selected ...
    image[:, 0, 0] = np.nan                                      # ... may hold anything
    assert not upstream[:, 0, 0].any()
    ordered = ref.grad_grid(image, upstream, Gx, Gy, L)
    value, magnitude, reach = ref.grad_grid64(np.nan_to_num(image), upstream, Gx, Gy, L, reach=True)
    assert np.all(np.isfinite(ordered))
    # The f32 coordinates: g = x * scale carries two roundings (<= 2 u (G-1) absolute in t, u = 2^-24), the luminance about
    # four, so each of the three weights is off by at most 4 u G and their product by 12 u G; a pixel's term then by that times
    # |g_i u_j|.  The products and the sums add a few u per term, far below 2e-6 of the terms' magnitudes for these sizes.
    u32 = 2.0 ** -24
    assert np.all(np.abs(ordered - value) <= 2e-6 * magnitude + 12 * u32 * max(Gx, Gy, L) * reach)
    # a vertex no pixel reaches holds exact zeros
    xs, ys = ref.cells(W, Gx), ref.cells(H, Gy)
    for iy in range(Gy):
        for ix in range(Gx):
            if xs[max(ix - 1, 0)] == xs[min(ix + 1, Gx - 1)] or ys[max(iy - 1, 0)] == ys[min(iy + 1, Gy - 1)]:
                assert not ordered[iy, ix].any() and not value[iy, ix].any()
    if size == (4, 4):                                           # (at 8x8 every second cell is empty, but no vertex's two are)
        assert sum(1 for ix in range(Gx) if xs[max(ix - 1, 0)] == xs[min(ix + 1, Gx - 1)]) > 0


def test_cells_partition_the_axis_and_agree_with_the_coordinates():
    for n, G in ((1, 2), (7, 5), (8, 16), (53, 3), (480, 64), (1920, 16), (1088, 2)):
        first = ref.cells(n, G)
        i0, t = ref.cell(n, G)
        assert first[0] == 0 and first[G - 1] == n and np.all(np.diff(first) >= 0)
        for c in range(G - 1):
            assert np.all(i0[first[c]:first[c + 1]] == c)
        assert np.all(t >= 0) and np.all(t <= np.float32(1) + np.float32(1e-6))
