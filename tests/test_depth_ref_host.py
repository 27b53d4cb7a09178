"""CPU: the float64 reference of depth supervision (tests/depth_ref.py) pinned to things outside it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import depth_ref as R


def _planes(h, w, seed, holes=True):
    g = torch.Generator().manual_seed(seed)
    Z = 1.0 + 4.0 * torch.rand(h, w, generator=g)
    D = Z * (1.0 + 0.2 * (torch.rand(h, w, generator=g) - 0.5))
    w_t = torch.rand(h, w, generator=g)
    w_p = torch.rand(h, w, generator=g)
    if holes:
        w_t[torch.rand(h, w, generator=g) < 0.3] = 0.0
        D[torch.rand(h, w, generator=g) < 0.1] = 0.0
    return D, Z, w_t, w_p


@pytest.mark.parametrize("size_in,size_full,crop", [((70, 150), (35, 75), (32, 64)), ((50, 96), (16, 48), (16, 48)), ((64, 64), (64, 64), (64, 64))])
def test_resample_without_holes_is_the_antialiased_resize(size_in, size_full, crop):
    rng = np.random.default_rng(1)
    src = rng.uniform(0.5, 9.0, size_in).astype(np.float32)
    depth, weight, den = R.resample(src, R.FORMAT_F32, size_full, crop, min_coverage=0.5)
    want = F.interpolate(torch.from_numpy(src).double()[None, None], size=size_full, mode="bilinear", antialias=True, align_corners=False)[0, 0]
    want = want[:crop[0], :crop[1]].numpy()
    assert np.abs(depth - want).max() < 1e-12 * 9.0
    assert np.abs(weight - 1.0).max() < 1e-12 and np.abs(den - 1.0).max() < 1e-12


def test_factor_one_is_the_identity_and_a_hole_stays_a_hole():
    rng = np.random.default_rng(2)
    src = rng.integers(1, 65536, (20, 33)).astype(np.uint16)
    src[3, 4] = 0
    src[10:13, 20:25] = 0
    depth, weight, _ = R.resample(src, R.FORMAT_U16, (20, 33), (16, 32), depth_scale=0.001, min_coverage=1.0)
    z = (src.astype(np.float32) * np.float32(0.001)).astype(np.float64)[:16, :32]
    assert np.array_equal(depth, np.where(src[:16, :32] != 0, z, 0.0))
    assert np.array_equal(weight, (src[:16, :32] != 0).astype(np.float64))
    f = np.full((8, 8), 2.0, np.float32)
    f[0, 0], f[1, 1], f[2, 2], f[3, 3] = np.nan, np.inf, -1.0, 0.0
    depth, weight, _ = R.resample(f, R.FORMAT_F32, (8, 8))
    assert np.all(np.isfinite(depth)) and weight.sum() == 60 and depth.sum() == 120.0


def test_a_hole_is_never_interpolated_across_and_coverage_gates_the_weight():
    src = np.full((8, 8), 3.0, np.float32)
    src[:, 4:] = np.nan                                    # the right half is a hole
    depth, weight, den = R.resample(src, R.FORMAT_F32, (4, 4), min_coverage=0.0)
    assert np.allclose(depth[:, :2], 3.0, atol=1e-12) and np.all(depth[:, 3] == 0) and np.all(weight[:, 3] == 0)
    assert np.all((den[:, 2] > 0) & (den[:, 2] < 0.5)) and np.allclose(depth[:, 2], 3.0, atol=1e-12)      # the mixed column: the valid mean
    _, weight_half, _ = R.resample(src, R.FORMAT_F32, (4, 4), min_coverage=0.5)
    assert np.all(weight_half[:, 2] == 0) and np.array_equal(weight_half[:, :2], weight[:, :2])


@pytest.mark.parametrize("flags", [R.ALIGN | R.L2, R.ALIGN, R.ALIGN | R.INVERT_PREDICTED, R.ALIGN | R.INVERT_PREDICTED | R.INVERT_TARGET | R.L2])
def test_a_planted_affine_map_is_recovered(flags):
    D, Z, w_t, w_p = _planes(24, 40, 3)
    a, b = 0.37, 0.21
    sel, _ = R.select(D, Z, w_t, w_p)
    x, y = R.spaces(D, Z, sel, flags, torch.float64)
    # a target whose y-space value satisfies x = a y + b exactly: plant it through Z
    y_planted = (x - b) / a
    Zp = torch.where(sel, 1.0 / y_planted if flags & R.INVERT_TARGET else y_planted, Z.double()).float()
    out = R.evaluate(D, Zp, w_t, w_p, flags)
    assert abs(out["terms"][2].item() - a) < 1e-5 and abs(out["terms"][3].item() - b) < 1e-5
    assert out["terms"][0].item() < 1e-5


def test_l2_aligned_gradient_is_the_total_derivative():
    """envelope theorem: with s, t held fixed the L2 gradient equals autograd through the fit, and central differences"""
    for flags in (R.ALIGN | R.L2, R.ALIGN | R.L2 | R.INVERT_PREDICTED, R.ALIGN | R.L2 | R.INVERT_PREDICTED | R.INVERT_TARGET):
        D, Z, w_t, w_p = _planes(9, 13, 4)
        out = R.evaluate(D, Z, w_t, w_p, flags, round_terms=False)
        Dd = D.double().requires_grad_(True)
        L = R.loss_through_fit(Dd, Z, w_t, w_p, flags)
        L.backward()
        assert abs(L.item() - out["terms"][0].item()) < 1e-14
        scale = out["grad"].abs().max().item()
        assert scale > 0 and (Dd.grad - out["grad"]).abs().max().item() < 1e-10 * scale
        # central differences of the helper's own loss, at a few selected pixels
        idx = torch.nonzero(out["selected"])[:6]
        for i, j in idx.tolist():
            h = 1e-4
            Dp, Dm = D.double().clone(), D.double().clone()
            Dp[i, j] += h
            Dm[i, j] -= h
            fd = (R.loss_through_fit(Dp, Z, w_t, w_p, flags) - R.loss_through_fit(Dm, Z, w_t, w_p, flags)).item() / (2 * h)
            assert abs(fd - out["grad"][i, j].item()) < 1e-6 * scale + 1e-9
        assert torch.all(out["grad"][~out["selected"]] == 0)


def test_l1_aligned_gradient_is_the_detached_one():
    flags = R.ALIGN
    D, Z, w_t, w_p = _planes(9, 13, 5)
    out = R.evaluate(D, Z, w_t, w_p, flags, round_terms=False)
    s, t = out["terms"][2], out["terms"][3]
    Dd = D.double().requires_grad_(True)
    sel, w32 = R.select(D, Z, w_t, w_p)
    x, y = R.spaces(Dd, Z, sel, flags, torch.float64)
    L = (w32.double() * (x - (s * y + t)).abs()).sum() / w32.double().sum()
    L.backward()
    assert (Dd.grad - out["grad"]).abs().max().item() < 1e-12


def test_degenerate_fits_give_zero_scale_and_the_mean():
    D, Z, w_t, _ = _planes(6, 7, 6, holes=False)
    constant = torch.full_like(Z, 2.5)
    out = R.evaluate(D, constant, w_t, None, R.ALIGN | R.L2)
    w = torch.where(w_t > 0, w_t, torch.zeros_like(w_t)).double()
    assert out["terms"][2].item() == 0.0
    assert abs(out["terms"][3].item() - ((w * D.double()).sum() / w.sum()).item()) < 1e-6
    one = torch.zeros_like(w_t)
    one[2, 3] = 0.7
    out = R.evaluate(D, Z, one, None, R.ALIGN)
    assert out["terms"][2].item() == 0.0 and out["terms"][4].item() == 1.0
    assert abs(out["terms"][3].item() - D[2, 3].item()) < 1e-6 and out["terms"][0].item() < 1e-6


def test_nothing_selected_gives_zeros_and_unusable_values_are_inert():
    D, Z, w_t, w_p = _planes(5, 6, 7)
    for flags in range(16):
        out = R.evaluate(D, Z, torch.zeros_like(w_t), w_p, flags)
        assert torch.all(out["terms"] == 0) and torch.all(out["grad"] == 0)
    base = R.evaluate(D, Z, w_t, w_p, 15)
    D2, Z2, w_t2, w_p2 = D.clone(), Z.clone(), w_t.clone(), w_p.clone()
    off = ~base["selected"]
    D2[off] = float("nan")
    Z2[off] = float("inf")
    w_t2[off] = -1.0
    w_p2[off] = float("nan")
    again = R.evaluate(D2, Z2, w_t2, w_p2, 15)
    assert torch.equal(again["terms"], base["terms"]) and torch.equal(again["grad"], base["grad"])
